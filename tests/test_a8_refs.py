"""``ops.a8_linear`` / ``ops.quantize_act_rows`` and ``Decoder(..., prefill_act="int8")`` where no GPU is: the op's
fallback is the W8A8 arithmetic written out in torch (the reference of ``nsa_a8_gemm``), and a CPU decoder in this
mode really quantizes its prompt activations."""

import pytest
import torch
import torch.nn.functional as F

from nanosandbox_amd import ops
from nanosandbox_amd.runtime.decode import Decoder
from test_decode_linear_refs import rand_linear
from test_quant_refs import _model


def a8_formula(x, q, scale, b, gelu):
    """The op's definition: int64 sum, then three separately rounded fp32 operations, the exact GELU, x's dtype."""
    xq, sx = ops.quantize_cache_rows(x)
    r = (xq.long() @ q.long().t()).float()
    r = r * sx[:, None]
    r = r * scale
    if b is not None:
        r = r + b.to(x.dtype).float()
    return (F.gelu(r) if gelu else r).to(x.dtype)


@pytest.mark.parametrize("M,N,K", [(3, 5, 64), (130, 33, 1600)])
@pytest.mark.parametrize("gelu", [False, True])
def test_a8_linear_fallback_is_the_formula(M, N, K, gelu):
    x, q, scale, b = rand_linear(M, N, K, True)
    w = ops.QuantWeight(q, scale)
    for xx in (x, x.float()):
        for bias in (None, b):
            y = ops.a8_linear(xx.view(1, M, K), w, bias, gelu=gelu)
            assert y.shape == (1, M, N) and y.dtype == xx.dtype and not y.requires_grad
            assert torch.equal(y[0], a8_formula(xx, q, scale, bias, gelu))
    got, want = ops.quantize_act_rows(x), ops.quantize_cache_rows(x)
    assert torch.equal(got[0], want.q) and torch.equal(got[1], want.scale)
    for bad in (ops.quantize_mxfp4(torch.randn(N, K)), torch.randn(N, K)):
        with pytest.raises(TypeError):
            ops.a8_linear(x, bad)


@pytest.mark.parametrize("K,measured", [(768, 7.6e-3), (3072, 8.6e-3)])
def test_a8_linear_error_against_the_weight_only_linear(K, measured):
    """The price of int8 activations: ||a8_linear - linear(x, dequantize(w))|| / ||linear|| on Gaussian rows.  A
    uniform rounding step of absmax / 127 predicts about 0.7 %; measured (fp32, CPU) 0.755 % at K = 768 and 0.860 % at
    K = 3072 (a wider row has a larger absmax); the bound is twice the measured figure."""
    x, q, scale, b = rand_linear(64, 96, K, True)
    w = ops.QuantWeight(q, scale)
    ref = ops.linear(x.float(), ops.dequantize(w), b.float())
    err = ((ops.a8_linear(x.float(), w, b.float()) - ref).norm() / ref.norm()).item()
    print(f"a8_linear K = {K}: relative error {err:.3e}")
    assert 0 < err <= 2 * measured


def test_prefill_act_refusals_and_cpu_decoder(tmp_path, monkeypatch):
    """ValueError without ``quantize_prefill``, on MXFP4 weights and for another value; ``fits`` tells the modes
    apart; the CPU decoder's prefill logits differ from the weight-only decoder's (measured relative distance on
    this model, fp32: 7.2e-3: the accuracy figure the README quotes) and stay within what its 8 block linears' own
    errors add up to at most (8 x 0.86 % = 6.9e-2); the ``sample.py`` key parses and refuses the same way."""
    from nanosandbox_amd import sample
    m = _model()
    idx = torch.randint(0, 97, (3, 20))
    on_kw = dict(quantize="int8", quantize_prefill=True, prefill_act="int8")
    for kw in (dict(quantize="int8", prefill_act="int8"), dict(on_kw, quantize="mxfp4"), dict(on_kw, prefill_act="fp8")):
        with pytest.raises(ValueError):
            Decoder(m, 3, use_graph=False, **kw)
        with pytest.raises(ValueError):
            m.generate_cached(idx[:, :4], 4, top_k=1, **kw)
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
    logits = {}
    for name, kw in (("off", dict(on_kw, prefill_act="")), ("on", on_kw)):
        d = Decoder(m, 3, use_graph=False, **kw)
        assert d.fits(3, **kw) and d.fits(3, **on_kw) == (name == "on")
        with torch.no_grad():
            logits[name] = d.prefill(idx)
        d.release()
    dist = ((logits["on"] - logits["off"]).norm() / logits["off"].norm()).item()
    print(f"prefill logits, a8 against weight-only int8 (CPU fp32): relative distance {dist:.3e}")
    assert 0 < dist < 6.9e-2
    ys = m.generate_batch([idx[0, :3], idx[1, :5], idx[2, :9]], 6, top_k=1, batch_size=2, **on_kw)
    assert [y.numel() for y in ys] == [9, 11, 15]

    args_model = dict(block_size=48, vocab_size=97, n_layer=2, n_head=4, n_embd=64, bias=True, dropout=0.0)
    (tmp_path / "prompt.txt").write_text("1,2,3")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    torch.save({"model": m.state_dict(), "model_args": args_model, "iter_num": 0, "best_val_loss": 0.0, "config": {}},
               tmp_path / "ckpt.pt")
    args = [f"--out_dir={tmp_path}", "--device=cpu", "--num_samples=1", "--max_new_tokens=6",
            f"--start=FILE:{tmp_path / 'prompt.txt'}", "--top_k=1", "--quantize=int8"]
    with pytest.raises(ValueError):
        sample.main(args + ["--prefill_act=int8"])
    with pytest.raises(ValueError):
        sample.main(args + ["--quantize_prefill=True", "--prefill_act=fp8"])
    assert len(sample.main(args + ["--quantize_prefill=True", "--prefill_act=int8"])[0].split(",")) == 9
