"""A shared prompt prefix, CPU side (fp32 torch paths): ``ops.prefix_attention`` against full
causal attention over the concatenated sequence, ``Decoder.prefill_suffixes`` and the steps after
it against the unshared per-row decoder, ``generate_batch(shared_prefix=True)`` against the
ordinary path with its argument checks and prefix reuse, and ``sample.py --shared_prefix``."""

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder, common_prefix_len


def _model():  # tests/test_shared_prompt_refs.py's
    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval()


def _small(block_size=48):  # tests/test_shared_prompt_refs.py's
    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=block_size, vocab_size=97, n_layer=2, n_head=4, n_embd=64, dropout=0.0,
                         bias=True)).eval()


def _close(a, b):  # tests/test_shared_prompt_refs.py's: within 1e-4 of the logits' norm
    return bool((a - b).norm() <= 1e-4 * b.norm())


def _greedy_gap_ok(m, prompt, n, quantize=None):  # tests/test_shared_prompt_refs.py's
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


# ---------------------------------------------------------------------------- 1. the op

@pytest.mark.parametrize("S", [1, 19])
@pytest.mark.parametrize("P", [1, 40])
def test_prefix_attention_equals_causal_attention_of_the_whole_sequence(P, S):
    B, H, Tp, D = 3, 4, 48, 64
    C = H * D
    torch.manual_seed(10 * P + S)
    full = torch.randn(B, P + S, 3 * C)
    full[:, :P] = full[:1, :P]  # one prefix for every row
    pkc, pvc = (torch.full((1, H, Tp, D), float("nan")) for _ in range(2))  # rows >= P are never used
    ops.kv_append(full[:1, :P], pkc, pvc, None, 0)
    qkv = full[:, P:].contiguous()
    q0, pk0, pv0 = qkv.clone(), pkc.clone(), pvc.clone()
    want = ops.attention(full, H, 0.0, False)[:, P:]  # fp32 causal attention; the outputs at positions P ..
    got = ops.prefix_attention(qkv, pkc, pvc, P, H)
    assert got.shape == (B, S, C) and got.dtype == qkv.dtype and not bool(got.isnan().any())
    assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), (got - want).abs().max()
    assert torch.equal(qkv, q0)  # no input is written
    assert torch.equal(pkc.isnan(), pk0.isnan()) and torch.equal(pkc[:, :, :P], pk0[:, :, :P])
    assert torch.equal(pvc.isnan(), pv0.isnan()) and torch.equal(pvc[:, :, :P], pv0[:, :, :P])


# ---------------------------------------------------------------------------- 2. the decoder

@torch.no_grad()
def test_shared_prefix_decoder_matches_unshared_decoder():
    """Teacher forcing with tokens drawn once: a 40-token prefix, suffixes of 1 / 7 / 19 tokens,
    24 steps, B = 3.  Row 1 draws the stop token after step 5 and is frozen from then on."""
    m = _model()
    B, P, n_new = 3, 40, 24
    lens = [1, 7, 19]
    S = max(lens)
    torch.manual_seed(1)
    prefix = torch.randint(0, 512, (P,))
    suf = torch.randint(0, 512, (B, S))  # row b's suffix: its first lens[b] tokens; the rest is padding
    toks = torch.randint(0, 512, (B, n_new))
    lengths = torch.tensor(lens)
    sh = Decoder(m, B, use_graph=False, per_row=True, shared_prompt=True, max_new=S + n_new)
    un = Decoder(m, B, use_graph=False, per_row=True)
    assert sh.pkc[0].shape == (1, 4, 256, 64) and sh.kc[0].shape == (B, 4, S + n_new, 64)
    sh.prefill_shared(prefix)
    a = sh.prefill_suffixes(suf, lengths)
    b = un.prefill(torch.cat([prefix[None].expand(B, -1), suf], dim=1), lengths + P)
    assert a.shape == b.shape == (B, 512) and _close(a, b), ((a - b).norm() / b.norm()).item()
    assert int(sh.plen) == P and sh.prefills == 1
    assert sh.positions == un.positions == [P + n for n in lens]
    for i in range(3):  # the prefix's rows are in the prompt cache, once; the suffixes' in the row caches
        for r in range(B):
            assert torch.allclose(sh.pkc[i][0, :, :P], un.kc[i][r, :, :P], atol=1e-5, rtol=1e-5)
            assert torch.allclose(sh.kc[i][r, :, :lens[r]], un.kc[i][r, :, P:P + lens[r]], atol=1e-5, rtol=1e-5)
    stop = None
    for t in range(n_new):
        tok = toks[:, t].clone()
        if t > 5:
            tok[1] = stop  # a finished row is fed its last token again
        a, b = sh.step(tok), un.step(tok)
        assert _close(a, b), (t, ((a - b).norm() / b.norm()).item())
        if t == 5:
            stop = int(b[1].argmax())
            assert stop not in (int(b[0].argmax()), int(b[2].argmax())), "pick another seed: rows 0 / 2 draw it too"
            for d, lg in ((sh, a), (un, b)):  # greedy draw with a stop token: row 1 finishes
                d.sample_into(lg, 1.0, 1, stop_token=stop)
                assert d.done.tolist() == [0, 1, 0]
    steps = [n_new, 6, n_new]
    assert sh.positions == un.positions == [P + n + s for n, s in zip(lens, steps)]
    for i in range(3):  # a row's suffix and fed tokens are in its slots 0 .., the prefix in none of them
        for r in range(B):
            n = lens[r] + steps[r]
            assert torch.allclose(sh.kc[i][r, :, :n], un.kc[i][r, :, P:P + n], atol=1e-5, rtol=1e-5)
    assert sh.prefills == 1
    sh.release()
    un.release()


@torch.no_grad()
def test_prefill_suffixes_without_lengths_and_its_argument_checks():
    m = _small()
    torch.manual_seed(5)
    prefix, suf = torch.randint(0, 97, (9,)), torch.randint(0, 97, (2, 4))
    sh = Decoder(m, 2, use_graph=False, shared_prompt=True, max_new=8)
    un = Decoder(m, 2, use_graph=False)
    with pytest.raises(AssertionError):  # no prefix yet
        sh.prefill_suffixes(suf)
    with pytest.raises(AssertionError):  # not a shared decoder
        un.prefill_suffixes(suf)
    sh.prefill_shared(prefix)
    with pytest.raises(AssertionError):  # lengths need per_row
        sh.prefill_suffixes(suf, torch.tensor([1, 4]))
    with pytest.raises(AssertionError):  # S <= R
        sh.prefill_suffixes(torch.randint(0, 97, (2, 9)))
    a = sh.prefill_suffixes(suf)
    b = un.prefill(torch.cat([prefix[None].expand(2, -1), suf], dim=1))
    assert _close(a, b) and sh.positions == un.positions == [13, 13]
    tok = torch.tensor([3, 5])
    assert _close(sh.step(tok), un.step(tok))
    sh.release()
    un.release()


# ---------------------------------------------------------------------------- 3. the front end

def test_common_prefix_len():
    t = torch.tensor
    assert common_prefix_len([t([1, 2, 3, 4]), t([1, 2, 3, 9, 9]), t([1, 2, 3])]) == 2  # the shortest keeps a token
    assert common_prefix_len([t([1, 2, 3, 4]), t([1, 2, 5, 4])]) == 2
    assert common_prefix_len([t([1, 2, 3]), t([1, 2, 3])]) == 2
    assert common_prefix_len([t([1, 2, 3]), t([4, 2, 3])]) == 0
    assert common_prefix_len([t([7]), t([7, 8])]) == 0


def _prompts(prefix, *suffixes):
    return [torch.cat([prefix, torch.tensor(s)]) for s in suffixes]


def test_generate_batch_shared_prefix():
    m = _small()
    torch.manual_seed(3)
    prefix = torch.randint(0, 97, (10,))
    prompts = _prompts(prefix, [5], [7, 11, 13, 2], [17, 19, 23, 29, 31, 37, 41])
    n_new = 20
    # greedy rows equal the ordinary path's, row for row, with and without int8 weights
    for q in (None, "int8"):
        assert all(_greedy_gap_ok(m, p, n_new, q) for p in prompts), "pick another seed: a near-tie in a greedy run"
        want = m.generate_batch(prompts, n_new, top_k=1, quantize=q)
        got = m.generate_batch(prompts, n_new, top_k=1, quantize=q, shared_prefix=True)
        assert len(got) == 3
        for p, u, v in zip(prompts, got, want):
            assert u.numel() == p.numel() + n_new and torch.equal(u, v), q
    want = m.generate_batch(prompts, n_new, top_k=1)
    # a stop token cuts a row as on the ordinary path
    stop = int(want[1][prompts[1].numel() + 4])
    cut = m.generate_batch(prompts, n_new, top_k=1, stop_token=stop)
    got = m.generate_batch(prompts, n_new, top_k=1, stop_token=stop, shared_prefix=True)
    assert all(torch.equal(u, v) for u, v in zip(got, cut)) and int(got[1][-1]) == stop
    assert got[1].numel() <= prompts[1].numel() + 5
    # identical prompts: the prefix is all but the last token
    same = m.generate_batch([prompts[1]] * 3, n_new, top_k=1, shared_prefix=True)
    assert all(torch.equal(y, want[1]) for y in same)
    # one prompt, or no common prefix: the ordinary path (a shared decoder handed in is not used)
    dec = Decoder(m, 2, use_graph=False, per_row=True, shared_prompt=True)
    other = prompts[2].flip(0)
    assert other[0] != prompts[0][0] and _greedy_gap_ok(m, other, n_new)
    ys = m.generate_batch([prompts[0], other], n_new, top_k=1, shared_prefix=True, decoder=dec)
    assert torch.equal(ys[0], want[0]) and torch.equal(ys[1], m.generate_batch([other], n_new, top_k=1)[0])
    assert dec.prefills == 0 and int(dec.pos.sum()) == 0
    dec.release()
    assert torch.equal(m.generate_batch([prompts[2]], n_new, top_k=1, shared_prefix=True)[0], want[2])
    # an unshared decoder handed to a shared_prefix call is replaced by a temporary one
    dec = Decoder(m, 3, use_graph=False, per_row=True)
    ys = m.generate_batch(prompts, n_new, top_k=1, shared_prefix=True, decoder=dec)
    assert all(torch.equal(u, v) for u, v in zip(ys, want)) and int(dec.pos.sum()) == 0
    dec.release()
    assert m.generate_batch(prompts, 0, shared_prefix=True)[0] is not None
    assert not [n for n, prm in m.named_parameters() if hasattr(prm, "compute")]


def test_shared_prefix_decoder_encodes_the_prefix_once():
    m = _small()
    torch.manual_seed(3)
    prefix = torch.randint(0, 97, (10,))
    first = _prompts(prefix, [5], [7, 11, 13, 2], [17, 19, 23])
    second = _prompts(prefix, [43, 47], [53], [59, 61, 67, 71])
    n_new = 12
    assert all(_greedy_gap_ok(m, p, n_new) for p in first + second), "pick another seed: a near-tie in a greedy run"
    dec = Decoder(m, 3, use_graph=False, per_row=True, shared_prompt=True, max_new=4 + n_new)
    a = m.generate_batch(first, n_new, top_k=1, shared_prefix=True, decoder=dec)
    assert dec.prefills == 1 and int(dec.plen) == 10
    b = m.generate_batch(second, n_new, top_k=1, shared_prefix=True, decoder=dec)
    assert dec.prefills == 1  # one prefix, different suffixes: it was not encoded again
    for ys, ps in ((a, first), (b, second)):
        for y, w in zip(ys, m.generate_batch(ps, n_new, top_k=1)):
            assert torch.equal(y, w)
    # a longer suffix than the row caches hold: a temporary decoder, this one untouched
    longer = _prompts(prefix, [5, 6, 7, 8, 9], [7])
    ys = m.generate_batch(longer + [first[2]], n_new, top_k=1, shared_prefix=True, decoder=dec)
    assert dec.prefills == 1 and [y.numel() for y in ys] == [27, 23, 25]
    dec.release()


def test_shared_prefix_refusals():
    m = _small()
    torch.manual_seed(2)
    prefix = torch.randint(0, 97, (10,))
    prompts = _prompts(prefix, [5], [7, 11])
    with pytest.raises(ValueError, match="kv_quantize"):
        m.generate_batch(prompts, 4, top_k=1, shared_prefix=True, kv_quantize="int8")
    with pytest.raises(ValueError, match="shared_prompt"):
        m.generate_batch(prompts, 4, top_k=1, shared_prefix=True, shared_prompt=True)
    with pytest.raises(ValueError, match="shared_prompt"):  # also for equal prompts
        m.generate_batch([prompts[0]] * 2, 4, top_k=1, shared_prefix=True, shared_prompt=True)
    with pytest.raises(ValueError, match="block_size"):  # 12 + 37 > 48: no recompute fallback
        m.generate_batch(prompts, 37, top_k=1, shared_prefix=True)
    assert len(m.generate_batch(prompts, 36, top_k=1, shared_prefix=True)[1]) == 48
    # what the shared-prompt form refuses, it still refuses
    with pytest.raises(ValueError):
        m.generate_batch(prompts, 4, top_k=1, shared_prompt=True)
    assert not [n for n, prm in m.named_parameters() if hasattr(prm, "compute")]


# ---------------------------------------------------------------------------- 4. sample.py

def test_sample_shared_prefix_with_prompts_file(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    m = _small()
    args_model = dict(block_size=48, vocab_size=97, n_layer=2, n_head=4, n_embd=64, bias=True, dropout=0.0)
    (tmp_path / "prompt.txt").write_text("1,2,3")
    (tmp_path / "prompts.txt").write_text("1,2,3,4,5,6\n1,2,3,4,9\n1,2,3,4,7,8,10\n")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    torch.save({"model": m.state_dict(), "model_args": args_model, "iter_num": 0, "best_val_loss": 0.0,
                "config": {}}, tmp_path / "ckpt.pt")
    args = [f"--out_dir={tmp_path}", "--device=cpu", "--max_new_tokens=12", f"--start=FILE:{tmp_path / 'prompt.txt'}",
            "--top_k=1", f"--prompts_file={tmp_path / 'prompts.txt'}"]
    assert sample.SAMPLE_DEFAULTS["shared_prefix"] is False
    with pytest.raises(ValueError, match="kv_cache"):
        sample.main(args + ["--shared_prefix=True", "--kv_cache=False"])
    with pytest.raises(ValueError, match="kv_quantize"):
        sample.main(args + ["--shared_prefix=True", "--kv_quantize=int8"])
    with pytest.raises(ValueError, match="shared_prompt"):
        sample.main(args[:-1] + ["--shared_prefix=True", "--shared_prompt=True", "--sample_batch=2"])
    for line in ("1,2,3,4,5,6", "1,2,3,4,9", "1,2,3,4,7,8,10"):
        assert _greedy_gap_ok(m, torch.tensor([int(t) for t in line.split(",")]), 12)
    want = sample.main(args + ["--num_samples=1"])
    assert len(want) == 3 and [len(t.split(",")) for t in want] == [18, 17, 19]
    prefills = []
    real = Decoder.prefill_shared
    monkeypatch.setattr(Decoder, "prefill_shared", lambda self, i: (real(self, i), prefills.append(
        (self.prefills, i.numel())))[0])
    got = sample.main(args + ["--shared_prefix=True", "--num_samples=2"])
    assert got == want + want
    assert prefills == [(1, 4), (1, 4)]  # two rounds on one decoder: the 4-token prefix was encoded once
