"""int8 weight-only decoding, CPU side: the row quantizer's properties, and a quantized
``Decoder`` (the dequantize fallback of the decode ops: the reference semantics of the int8
kernels) against the model whose weights are ``dequantize(quantize_rows_int8(W))``."""

import copy

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder


def _model(bias=True, n_layer=2, n_head=4, n_embd=64, block_size=48, vocab_size=97):  # tests/test_decode.py's
    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=block_size, vocab_size=vocab_size, n_layer=n_layer, n_head=n_head,
                         n_embd=n_embd, dropout=0.0, bias=bias)).eval()


def _quant_params(m):
    """The five quantized weight groups: c_attn, attention c_proj, c_fc, MLP c_proj of every
    block, and the tied lm_head / wte table."""
    ps = []
    for blk in m.transformer.h:
        ps += [blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight]
    return ps + [m.lm_head.weight]


def _dequantized_copy(m):
    """A deep copy whose quantized weight groups hold dequantize(quantize_rows_int8(w))."""
    m2 = copy.deepcopy(m)
    assert m2.lm_head.weight is m2.transformer.wte.weight
    with torch.no_grad():
        for p in _quant_params(m2):
            p.copy_(ops.dequantize(ops.quantize_rows_int8(p)))
    return m2


@pytest.mark.parametrize("N,K,mul", [(100, 64, 1.0), (16, 64, 3.0), (4800, 1600, 1.0)])
def test_quantizer_properties(N, K, mul):
    torch.manual_seed(N + K)
    w = torch.randn(N, K) * 0.05 * mul
    w[3] = 0.0
    w[5] = 0.37
    qw = ops.quantize_rows_int8(w)
    assert isinstance(qw, ops.QuantWeight) and isinstance(qw, tuple)
    q, scale = qw
    assert q.dtype == torch.int8 and q.shape == (N, K) and q.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == (N,)
    assert int(q.min()) >= -127 and int(q.max()) <= 127
    absmax = w.abs().amax(dim=1)
    nz = absmax > 0
    assert torch.equal(scale[nz], (absmax / 127)[nz])
    assert bool((q[3] == 0).all()) and float(scale[3]) == 1.0
    assert bool((q[5] == 127).all())
    assert bool((q[nz].abs().amax(dim=1) == 127).all())  # every non-zero row uses the full range
    # round-to-nearest: at most half a step away (the slack covers the fp32 division)
    err = (w.double() - q.double() * scale.double()[:, None]).abs()
    assert bool((err <= 0.5 * scale.double()[:, None] * (1 + 1e-4)).all()), (err / scale.double()[:, None]).max()
    assert torch.equal(ops.dequantize(qw), q.float() * scale[:, None])
    assert ops.dequantize(qw).dtype == torch.float32


@pytest.mark.parametrize("bias", [True, False])
def test_quantized_decoder_runs_the_dequantized_model(bias):
    m = _model(bias=bias)
    m2 = _dequantized_copy(m)
    # earlier shadows on quantized parameters (a trained model's optimizer shadows): replaced
    # while the decoder lives (the junk one would wreck the logits), back afterwards
    sentinel = torch.zeros(1)
    m.lm_head.weight.compute = sentinel
    kept = m.transformer.h[0].mlp.c_fc.weight.detach().clone()
    m.transformer.h[0].mlp.c_fc.weight.compute = kept
    idx = torch.randint(0, 97, (3, 20))
    full = m2.forward_logits(idx)  # [B, T, V]
    dec = Decoder(m, 3, use_graph=False, quantize="int8")
    with torch.no_grad():
        lg = dec.prefill(idx[:, :8])
        assert torch.allclose(lg, full[:, 7], atol=1e-4, rtol=1e-4)
        for t in range(8, 20):
            lg = dec.step(idx[:, t])
            assert torch.allclose(lg, full[:, t], atol=1e-4, rtol=1e-4), t
    assert dec.position == 20
    dec.release()
    assert m.lm_head.weight.compute is sentinel
    assert m.transformer.h[0].mlp.c_fc.weight.compute is kept
    del m.lm_head.weight.compute, m.transformer.h[0].mlp.c_fc.weight.compute
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
    # and with no shadow before: none after
    dec = Decoder(m, 3, use_graph=False, quantize="int8")
    assert hasattr(m.lm_head.weight, "compute")
    dec.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_quantized_greedy_tokens():
    m = _model()
    m2 = _dequantized_copy(m)
    idx = torch.randint(0, 97, (2, 5))
    a = m2.generate(idx, 30, top_k=1)
    b = m.generate_cached(idx, 30, top_k=1, quantize="int8")
    assert torch.equal(a, b)
    prompts = [torch.randint(0, 97, (n,)) for n in (3, 5, 9)]
    ya = m2.generate_batch(prompts, 30, top_k=1)
    yb = m.generate_batch(prompts, 30, top_k=1, quantize="int8")
    assert len(ya) == len(yb) == 3
    for p, u, v in zip(prompts, ya, yb):
        assert torch.equal(u, v) and v.numel() == p.numel() + 30
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_quantize_argument_checks(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    m = _model()
    idx = torch.randint(0, 97, (1, 10))
    with pytest.raises(ValueError):
        Decoder(m, 1, use_graph=False, quantize="int4")
    with pytest.raises(ValueError):
        m.generate_cached(idx, 4, top_k=1, quantize="int4")
    # prompt + new tokens past block_size: the recompute loop cannot run the quantized model
    with pytest.raises(ValueError):
        m.generate_cached(idx, 48, top_k=1, quantize="int8")
    with pytest.raises(ValueError):
        m.generate_batch([idx[0], idx[0, :3]], 48, top_k=1, quantize="int8")

    args_model = dict(block_size=48, vocab_size=97, n_layer=2, n_head=4, n_embd=64, bias=True, dropout=0.0)
    (tmp_path / "prompt.txt").write_text("1,2,3")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    outs = {}
    for name, mod in (("m", m), ("m2", _dequantized_copy(m))):
        d = tmp_path / name
        d.mkdir()
        torch.save({"model": mod.state_dict(), "model_args": args_model, "iter_num": 0, "best_val_loss": 0.0,
                    "config": {}}, d / "ckpt.pt")
        outs[name] = [f"--out_dir={d}", "--device=cpu", "--num_samples=1", "--max_new_tokens=12",
                      f"--start=FILE:{tmp_path / 'prompt.txt'}", "--top_k=1"]
    with pytest.raises(ValueError):
        sample.main(outs["m"] + ["--quantize=int8", "--kv_cache=False"])
    with pytest.raises(ValueError):
        sample.main(outs["m"] + ["--quantize=int4"])
    got = sample.main(outs["m"] + ["--quantize=int8"])
    want = sample.main(outs["m2"])
    assert got == want and len(got[0].split(",")) == 15
