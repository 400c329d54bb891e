"""Shared prompt caches, CPU side (fp32 torch paths): ``ops.decode_attention_shared`` against
``ops.decode_attention`` on caches that repeat the prompt in every row, the
``Decoder(shared_prompt=True)`` step against the unshared decoder, the argument checks of the
front ends and the reuse of an encoded prompt."""

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder


def _model():  # tests/test_decode_gpu.py's, in fp32 on the CPU
    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval()


def _small(block_size=48):  # tests/test_quant_refs.py's
    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=block_size, vocab_size=97, n_layer=2, n_head=4, n_embd=64, dropout=0.0,
                         bias=True)).eval()


# ---------------------------------------------------------------------------- 1. the op

@pytest.mark.parametrize("append", [False, True])
@pytest.mark.parametrize("offs", [[0], [1], [7], [0, 1, 7], [7, 0, 1]])
@pytest.mark.parametrize("P", [1, 5, 33])
def test_shared_op_equals_unshared_attention(P, offs, append):
    """One entry in ``offs``: a shared position; three: one per row."""
    B, H, Tp, R, D = 3, 4, 40, 12, 64
    C = H * D
    torch.manual_seed(100 * P + sum(offs))
    pkc, pvc = torch.randn(1, H, Tp, D), torch.randn(1, H, Tp, D)
    kc, vc = torch.randn(B, H, R, D), torch.randn(B, H, R, D)
    qkv = torch.randn(B, 1, 3 * C)
    plen = torch.tensor([P])
    pos = torch.tensor([P + o for o in offs])
    # the unshared caches: the prompt's rows copied into every batch row, then the row's own
    fk = torch.cat([pkc[:, :, :P].expand(B, -1, -1, -1), kc], dim=2).contiguous()
    fv = torch.cat([pvc[:, :, :P].expand(B, -1, -1, -1), vc], dim=2).contiguous()
    pk0, pv0, kc0, vc0 = pkc.clone(), pvc.clone(), kc.clone(), vc.clone()
    want = ops.decode_attention(qkv, fk, fv, pos, H, append=append)
    got = ops.decode_attention_shared(qkv, pkc, pvc, kc, vc, plen, pos, H, append=append)
    assert got.shape == (B, 1, C) and got.dtype == qkv.dtype
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), (got - want).abs().max()
    assert torch.equal(pkc, pk0) and torch.equal(pvc, pv0)  # the prompt caches are never written
    if not append:
        assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
        return
    k, v = qkv.view(B, 3, H, D)[:, 1], qkv.view(B, 3, H, D)[:, 2]
    for b, o in enumerate(offs * (1 if len(offs) > 1 else B)):
        assert torch.equal(kc[b, :, o], k[b]) and torch.equal(vc[b, :, o], v[b])  # slot pos - P
        kc0[b, :, o], vc0[b, :, o] = k[b], v[b]
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)  # and nothing else
    assert torch.equal(kc, fk[:, :, P:]) and torch.equal(vc, fv[:, :, P:])


def test_shared_op_row_past_its_cache():
    """A slot >= R stores nothing and the row attends over the prompt alone."""
    B, H, Tp, R, D, P = 2, 4, 16, 4, 64, 9
    torch.manual_seed(3)
    pkc, pvc = torch.randn(1, H, Tp, D), torch.randn(1, H, Tp, D)
    kc, vc = torch.randn(B, H, R, D), torch.randn(B, H, R, D)
    kc0 = kc.clone()
    qkv = torch.randn(B, 1, 3 * H * D)
    got = ops.decode_attention_shared(qkv, pkc, pvc, kc, vc, torch.tensor([P]), torch.tensor([P + 2, P + R]), H,
                                      append=True)
    q = qkv.view(B, 3, H, D)[1, 0]
    att = torch.softmax(torch.einsum("hd,hkd->hk", q, pkc[0, :, :P]) / 8.0, dim=-1)
    assert torch.allclose(got[1, 0].view(H, D), torch.einsum("hk,hkd->hd", att, pvc[0, :, :P]), atol=1e-5, rtol=1e-5)
    assert torch.equal(kc[1], kc0[1]) and not torch.equal(kc[0], kc0[0])


# ---------------------------------------------------------------------------- 2. the decoder

def _close(a, b):  # within 1e-4 of the logits' norm
    return bool((a - b).norm() <= 1e-4 * b.norm())


@pytest.mark.parametrize("per_row", [False, True])
@torch.no_grad()
def test_shared_decoder_matches_unshared_decoder(per_row):
    """Teacher forcing with tokens drawn once, so near-ties cannot make the two diverge: 24 steps
    after a 40-token prompt, B = 3.  per_row: row 1 draws the stop token after step 5 and is
    frozen from then on: it keeps its position and its slot while the others go on."""
    m = _model()
    B, T0, n_new = 3, 40, 24
    torch.manual_seed(1)
    prompt = torch.randint(0, 512, (T0,))
    toks = torch.randint(0, 512, (B, n_new))
    sh = Decoder(m, B, use_graph=False, per_row=per_row, shared_prompt=True, max_new=n_new)
    un = Decoder(m, B, use_graph=False, per_row=per_row)
    assert sh.shared and sh.R == n_new and sh.pkc[0].shape == (1, 4, 256, 64) and sh.kc[0].shape == (B, 4, n_new, 64)
    a, b = sh.prefill_shared(prompt), un.prefill(prompt[None].expand(B, -1).contiguous())
    assert a.shape == b.shape == (B, 512) and _close(a, b)
    assert int(sh.plen) == T0 and sh.positions == [T0] * B and sh.prefills == 1
    for i in range(3):  # the prompt's rows are in the prompt cache, once
        assert torch.allclose(sh.pkc[i][0, :, :T0], un.kc[i][1, :, :T0], atol=1e-5, rtol=1e-5)
    frozen_slot = stop = None
    for t in range(n_new):
        tok = toks[:, t].clone()
        if per_row and t > 5:
            tok[1] = stop  # a finished row is fed its last token again
        a, b = sh.step(tok), un.step(tok)
        assert _close(a, b), (t, ((a - b).norm() / b.norm()).item())
        if per_row and t == 5:
            stop = int(b[1].argmax())
            assert stop not in (int(b[0].argmax()), int(b[2].argmax())), "pick another seed: rows 0 / 2 draw it too"
            for d, lg in ((sh, a), (un, b)):  # greedy draw with a stop token: row 1 finishes
                d.sample_into(lg, 1.0, 1, stop_token=stop)
                assert d.done.tolist() == [0, 1, 0]
        if per_row and t == 6:
            frozen_slot = sh.kc[1][1, :, 6].clone()
    if per_row:
        assert sh.positions == un.positions == [T0 + n_new, T0 + 6, T0 + n_new]
        assert torch.equal(sh.kc[1][1, :, 6], frozen_slot) and bool(frozen_slot.abs().sum() > 0)
        assert bool((sh.kc[1][1, :, 7:] == 0).all())  # nothing past the frozen row's slot
    else:
        assert sh.positions == un.positions == [T0 + n_new] * B
    for i in range(3):  # a row's own tokens are in its slots 0 ..
        assert torch.allclose(sh.kc[i][0], un.kc[i][0, :, T0:T0 + n_new], atol=1e-5, rtol=1e-5)
    sh.release()
    un.release()


# ---------------------------------------------------------------------------- 3. arguments

def _greedy_gap_ok(m, prompt, n, quantize=None):
    """No step of the unshared greedy run has its top two logits closer than 1e-4 of the logits'
    norm (the agreement bound of the two decoders): greedy texts can then be compared."""
    with torch.no_grad():
        dec = Decoder(m, 1, use_graph=False, quantize=quantize)
        lg = dec.prefill(prompt[None])
        ok = True
        for _ in range(n):
            top = torch.topk(lg[0], 2).values
            ok &= bool(top[0] - top[1] > 1e-4 * lg[0].norm())
            lg = dec.step(lg.argmax(dim=-1))
        dec.release()
    return ok


def test_shared_prompt_argument_checks(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    m = _small()
    torch.manual_seed(2)
    idx = torch.randint(0, 97, (1, 10))
    p, other = idx[0], idx[0].flip(0)
    with pytest.raises(ValueError):  # unequal prompts
        m.generate_batch([p, p, other], 4, top_k=1, shared_prompt=True)
    with pytest.raises(ValueError):
        m.generate_batch([p, p[:5]], 4, top_k=1, shared_prompt=True)
    with pytest.raises(ValueError):
        m.generate_cached(torch.stack([p, other]), 4, top_k=1, shared_prompt=True)
    with pytest.raises(ValueError):  # no int8 caches in the shared form
        m.generate_batch([p, p], 4, top_k=1, shared_prompt=True, kv_quantize="int8")
    with pytest.raises(ValueError):
        m.generate_cached(idx.expand(2, -1), 4, top_k=1, shared_prompt=True, kv_quantize="int8")
    with pytest.raises(ValueError):
        Decoder(m, 2, use_graph=False, shared_prompt=True, kv_quantize="int8")
    with pytest.raises(ValueError):  # nothing to share
        Decoder(m, 1, use_graph=False, shared_prompt=True)
    with pytest.raises(ValueError):  # prompt + new tokens past block_size: no recompute fallback
        m.generate_batch([p, p], 48, top_k=1, shared_prompt=True)
    with pytest.raises(ValueError):
        m.generate_cached(idx.expand(2, -1), 48, top_k=1, shared_prompt=True)
    # within block_size both run; greedy rows equal the ordinary path's, a single prompt goes that way
    assert _greedy_gap_ok(m, p, 20) and _greedy_gap_ok(m, p, 20, "int8")
    want = m.generate_cached(idx, 20, top_k=1)[0]
    for q in (None, "int8"):
        w = want if q is None else m.generate_cached(idx, 20, top_k=1, quantize=q)[0]
        ys = m.generate_batch([p, p, p], 20, top_k=1, shared_prompt=True, quantize=q)
        assert len(ys) == 3 and all(torch.equal(y, w) for y in ys), q
    y = m.generate_cached(idx.expand(2, -1), 20, top_k=1, shared_prompt=True)
    assert y.shape == (2, 30) and torch.equal(y[0], want) and torch.equal(y[1], want)
    assert torch.equal(m.generate_batch([p], 20, top_k=1, shared_prompt=True)[0], want)
    # an unshared decoder passed to a shared call (and the other way round) is replaced by a temporary one
    dec = Decoder(m, 2, use_graph=False, per_row=True)
    ys = m.generate_batch([p, p], 20, top_k=1, shared_prompt=True, decoder=dec)
    assert torch.equal(ys[1], want) and int(dec.pos.sum()) == 0
    dec.release()
    dec = Decoder(m, 2, use_graph=False, per_row=True, shared_prompt=True)
    ys = m.generate_batch([p, p[:4]], 20, top_k=1, decoder=dec)
    assert torch.equal(ys[0], want) and dec.prefills == 0
    dec.release()
    assert not [n for n, prm in m.named_parameters() if hasattr(prm, "compute")]

    args_model = dict(block_size=48, vocab_size=97, n_layer=2, n_head=4, n_embd=64, bias=True, dropout=0.0)
    (tmp_path / "prompt.txt").write_text("1,2,3")
    (tmp_path / "prompts.txt").write_text("1,2,3\n4,5\n")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    torch.save({"model": m.state_dict(), "model_args": args_model, "iter_num": 0, "best_val_loss": 0.0,
                "config": {}}, tmp_path / "ckpt.pt")
    args = [f"--out_dir={tmp_path}", "--device=cpu", "--max_new_tokens=12", f"--start=FILE:{tmp_path / 'prompt.txt'}",
            "--top_k=1"]
    assert sample.SAMPLE_DEFAULTS["shared_prompt"] is False
    with pytest.raises(ValueError, match="prompts_file"):
        sample.main(args + ["--shared_prompt=True", f"--prompts_file={tmp_path / 'prompts.txt'}"])
    with pytest.raises(ValueError, match="kv_cache"):
        sample.main(args + ["--shared_prompt=True", "--kv_cache=False", "--sample_batch=3"])
    with pytest.raises(ValueError, match="kv_quantize"):
        sample.main(args + ["--shared_prompt=True", "--kv_quantize=int8", "--sample_batch=3"])
    assert _greedy_gap_ok(m, torch.tensor([1, 2, 3]), 12)
    want = sample.main(args + ["--num_samples=1"])
    assert len(want) == 1 and len(want[0].split(",")) == 15 and want[0].startswith("1,2,3,")
    prefills = []
    real = Decoder.prefill_shared
    monkeypatch.setattr(Decoder, "prefill_shared", lambda self, i: (real(self, i), prefills.append(self.prefills))[0])
    got = sample.main(args + ["--shared_prompt=True", "--sample_batch=3", "--num_samples=6"])
    assert len(got) == 6 and all(t == want[0] for t in got)
    assert prefills == [1, 1]  # two rounds of three on one decoder: the prompt was encoded once
    # a last round of one sample goes the ordinary way
    got = sample.main(args + ["--shared_prompt=True", "--sample_batch=3", "--num_samples=4"])
    assert len(got) == 4 and all(t == want[0] for t in got)


# ---------------------------------------------------------------------------- 4. prompt reuse

def test_shared_decoder_encodes_a_prompt_once():
    m = _small()
    torch.manual_seed(4)
    p, other = torch.randint(0, 97, (10,)), torch.randint(0, 97, (7,))
    dec = Decoder(m, 4, use_graph=False, per_row=True, shared_prompt=True, max_new=16)
    assert dec.prefills == 0
    a = m.generate_batch([p] * 4, 16, temperature=1.0, shared_prompt=True, decoder=dec)
    b = m.generate_batch([p] * 4, 16, temperature=1.0, shared_prompt=True, decoder=dec)
    assert dec.prefills == 1
    for ys in (a, b):
        assert all(y.numel() == 26 and torch.equal(y[:10], p) for y in ys)
        assert all(0 <= int(y.min()) and int(y.max()) < 97 for y in ys)
    assert not all(torch.equal(x, y) for x, y in zip(a, b))  # a fresh salt per call
    assert not all(torch.equal(a[0], y) for y in a[1:])      # and the rows draw independently
    c = m.generate_batch([other] * 4, 16, temperature=1.0, shared_prompt=True, decoder=dec)
    assert dec.prefills == 2 and all(torch.equal(y[:7], other) for y in c)
    m.generate_batch([p] * 4, 16, temperature=1.0, shared_prompt=True, decoder=dec)
    assert dec.prefills == 3  # one prompt is kept, not a history
    # more new tokens than the row caches hold: a temporary decoder, this one untouched
    ys = m.generate_batch([p] * 4, 20, top_k=1, shared_prompt=True, decoder=dec)
    assert dec.prefills == 3 and all(y.numel() == 30 for y in ys)
    dec.release()
