"""Per-row positions, stop token and finished flag on MI355X: the per-row decode kernels
against fp32 torch, and the per-row graph-replayed step against the eager one and the full
fused forward (runtime/decode.py ``Decoder(per_row=True)``, ``GPT.generate_batch``)."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _model():
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


def test_per_row_attention_kernel(kernels):
    from nanosandbox_amd import ops

    torch.manual_seed(0)
    B, H, D, T = 4, 2, 64, 520  # three 256-key chunks, the last one partial
    C = H * D
    positions = [0, 255, 256, 519]
    kc = torch.randn(B, H, T, D, device=DEV).to(BF)
    vc = torch.randn(B, H, T, D, device=DEV).to(BF)
    qkv = torch.randn(B, 1, 3 * C, device=DEV).to(BF)
    kc0, vc0 = kc.clone(), vc.clone()
    pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
    y = ops.decode_attention(qkv, kc, vc, pos, H, append=True).float().view(B, H, D)
    q, k_new, v_new = qkv.view(B, 3, H, D).unbind(1)
    for b, p in enumerate(positions):
        # the one stored row, bitwise; everything else untouched
        assert torch.equal(kc[b, :, p], k_new[b]) and torch.equal(vc[b, :, p], v_new[b])
        kc0[b, :, p], vc0[b, :, p] = k_new[b], v_new[b]
        k, v = kc[b, :, :p + 1].float(), vc[b, :, :p + 1].float()
        att = torch.softmax(torch.einsum("hd,hkd->hk", q[b].float(), k) / math.sqrt(D), dim=-1)
        ref = torch.einsum("hk,hkd->hd", att, v)
        err = ((y[b] - ref).norm() / ref.norm()).item()
        assert err < 1e-2, (b, err)
    assert torch.equal(kc, kc0) and torch.equal(vc, vc0)
    # equal positions: the per-row form is the shared-position form, bit for bit
    ka, va, kb, vb = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    y_rows = ops.decode_attention(qkv, ka, va, torch.full((B,), 300, device=DEV, dtype=torch.int64), H, append=True)
    y_one = ops.decode_attention(qkv, kb, vb, torch.tensor([300], device=DEV, dtype=torch.int64), H, append=True)
    assert torch.equal(y_rows, y_one) and torch.equal(ka, kb) and torch.equal(va, vb)


def test_per_row_sampling_kernel(kernels):
    from nanosandbox_amd import ops

    torch.manual_seed(1)
    B, V = 4, 512
    logits = torch.randn(B, V, device=DEV) * 3.0
    am = logits.argmax(1)
    positions = [3, 9, 9, 40]
    pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
    done = torch.tensor([0, 0, 1, 0], device=DEV, dtype=torch.int64)
    tok = torch.full((B, 1), 777, device=DEV, dtype=torch.int64)
    gen = torch.full((B, 48), -5, device=DEV, dtype=torch.int64)
    ops.sample_topk_(logits, 1.0, 1, 99, pos, tok, gen, stop_token=int(am[1]), done=done)
    want_gen = torch.full((B, 48), -5, device=DEV, dtype=torch.int64)
    for b in (0, 1, 3):
        want_gen[b, positions[b]] = am[b]
        assert int(tok[b]) == int(am[b])
    assert int(tok[2]) == 777  # the finished row changes nothing
    assert torch.equal(gen, want_gen)
    stops = [1 if int(am[b]) == int(am[1]) else 0 for b in range(B)]
    assert done.tolist() == [stops[0], 1, 1, stops[3]] and done.tolist()[1] == 1
    # equal positions, no flags: the per-row draw is the shared-position draw
    t1, t2 = torch.zeros_like(tok), torch.zeros_like(tok)
    g1, g2 = torch.zeros_like(gen), torch.zeros_like(gen)
    ops.sample_topk_(logits, 0.8, 50, 99, torch.full((B,), 9, device=DEV, dtype=torch.int64), t1, g1)
    ops.sample_topk_(logits, 0.8, 50, 99, torch.tensor([9], device=DEV, dtype=torch.int64), t2, g2)
    assert torch.equal(t1, t2) and torch.equal(g1, g2)


@pytest.mark.parametrize("lens", [(5, 40, 33), (40,)])
def test_per_row_graph_decode_matches_eager_and_full_forward(kernels, lens):
    """B = 3: skinny GEMMs + the per-row attention; B = 1: the fused single-row path."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    B, steps = len(lens), 24
    seqs = [torch.randint(0, 512, (n + steps,)).to(DEV) for n in lens]
    idx = torch.zeros(B, max(lens), dtype=torch.int64, device=DEV)
    for b, n in enumerate(lens):
        idx[b, :n] = seqs[b][:n]
        idx[b, n:] = 17 + b  # right padding
    lengths = torch.tensor(lens, device=DEV)
    with torch.no_grad():
        full = [m.forward_logits(s[None])[0] for s in seqs]
        dg = Decoder(m, B, use_graph=True, per_row=True)
        de = Decoder(m, B, use_graph=False, per_row=True)
        lg, le = dg.prefill(idx, lengths), de.prefill(idx, lengths)
        assert torch.equal(lg, le)
        for b, n in enumerate(lens):
            assert ((lg[b] - full[b][n - 1]).norm() / full[b][n - 1].norm()).item() < 3e-2
        for t in range(steps):
            tok = torch.stack([seqs[b][n + t] for b, n in enumerate(lens)])
            lg = dg.step(tok).clone()
            le = de.step(tok)
            assert torch.equal(lg, le), t
            for b, n in enumerate(lens):
                ref = full[b][n + t]
                err = ((lg[b] - ref).norm() / ref.norm()).item()
                assert err < 3e-2, (b, t, err)
    assert dg.replays == steps
    assert dg.positions == de.positions == [n + steps for n in lens]
    dg.release()
    de.release()


def test_generate_batch_equal_lengths_is_generate_cached(kernels):
    m = _model()
    idx = torch.randint(0, 512, (3, 16), device=DEV)
    a = m.generate_batch(list(idx), 40, top_k=1, use_graph=True)
    b = m.generate_cached(idx, 40, top_k=1, use_graph=True)
    assert torch.equal(torch.stack(a), b)


def test_single_row_stop_token_ends_the_run_early(kernels):
    """B = 1 (the fused single-row step, sample.py's --stop_token with one sample): the row
    stops at the stop token, and run() leaves its replay loop once every row has finished."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    torch.manual_seed(6)
    prompt, n = torch.randint(0, 512, (5,)).to(DEV), 40
    free = m.generate_batch([prompt], n, top_k=1, use_graph=True)[0]
    new = free[5:].tolist()
    stop = next((t for k, t in enumerate(new[:16]) if new.index(t) == k >= 1), None)
    assert stop is not None, new  # a token first drawn as the 2nd .. 16th new one
    want = free[:5 + new.index(stop) + 1]
    dec = Decoder(m, 1, use_graph=True, per_row=True)
    try:
        out = m.generate_batch([prompt], n, top_k=1, stop_token=stop, decoder=dec)[0]
        assert dec.done.tolist() == [1] and dec.positions == [5 + new.index(stop)]
        assert dec.replays < n - 1  # the flags are read every 16 replays
    finally:
        dec.release()
    assert torch.equal(out, want)
    assert torch.equal(m.generate_batch([prompt], n, top_k=1, stop_token=stop, use_graph=False)[0], want)


def test_generate_batch_stop_token_under_the_graph(kernels):
    m = _model()
    torch.manual_seed(6)
    lens, n = (5, 40, 33), 40
    prompts = [torch.randint(0, 512, (k,)).to(DEV) for k in lens]  # host RNG: the same prompts everywhere
    free = m.generate_batch(prompts, n, top_k=1, use_graph=True)
    assert all(torch.equal(a, b) for a, b in zip(free, m.generate_batch(prompts, n, top_k=1, use_graph=False)))
    new = [f[k:].tolist() for f, k in zip(free, lens)]
    assert all(len(x) == n for x in new)
    # a stop token: some row's k-th new token (2 <= k < 40) that another row never emits
    stop = next((x[k - 1] for x in new for k in range(2, n)
                 if x.index(x[k - 1]) >= 1 and any(x[k - 1] not in y for y in new)), None)
    assert stop is not None, new
    outs = {g: m.generate_batch(prompts, n, top_k=1, stop_token=stop, use_graph=g) for g in (True, False)}
    stopped = 0
    for b, k in enumerate(lens):
        want = free[b] if stop not in new[b] else free[b][:k + new[b].index(stop) + 1]
        stopped += stop in new[b]
        assert torch.equal(outs[True][b], want), b
        assert torch.equal(outs[False][b], want), b
    assert 1 <= stopped < len(lens)
    assert not any(hasattr(p, "compute") for p in m.parameters())  # shadows released
