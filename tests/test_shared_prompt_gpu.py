"""Shared prompt caches on MI355X: the shared-prompt attention kernel against an fp32 reference
and against the unshared kernel on materialised caches, the ``Decoder(shared_prompt=True)``
step against the full fused forward, one captured graph for prompts of two lengths, and the
batch front end with sampling, stop tokens and int8 weights."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
H, D, TP, R = 4, 64, 704, 512  # TP: 5.5 prompt chunks of 128 keys; R: two row chunks of 256
OFFS = [0, 5, 255, 256]        # row offsets pos - P: first slot, inside, last of a chunk, first of the next


def _model():  # tests/test_decode_gpu.py's
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


_CACHES = {}


def _caches(B):
    """Random bf16 prompt and row caches, made once per batch size and never written: every run
    works on clones."""
    if B not in _CACHES:
        g = torch.Generator(device=DEV).manual_seed(1000 + B)
        _CACHES[B] = tuple(torch.randn(s, device=DEV, generator=g).to(BF)
                           for s in ((1, H, TP, D), (1, H, TP, D), (B, H, R, D), (B, H, R, D)))
    return _CACHES[B]


def _run_shared(qkv, pk, pv, kc, vc, P, pos, append):
    """The entry point itself with ``ws`` and ``out`` full of NaN -> (out [B, H, D] fp32, ws)."""
    from nanosandbox_amd.ops import _lib

    B = qkv.shape[0]
    n_split = -(-TP // 128) + -(-R // 256)
    ws = torch.full((B * H * n_split, 4 + D), float("nan"), device=DEV, dtype=torch.float32)
    out = torch.full((B, 1, H * D), float("nan"), device=DEV, dtype=BF)
    plen = torch.tensor([P], device=DEV, dtype=torch.int64)
    _lib.call("nsa_decode_attn_shared_rows" if pos.numel() > 1 else "nsa_decode_attn_shared", _lib.ptr(qkv),
              _lib.ptr(pk), _lib.ptr(pv), _lib.ptr(kc), _lib.ptr(vc), _lib.ptr(plen), _lib.ptr(pos), _lib.ptr(ws),
              _lib.ptr(out), B, H, TP, R, 1.0 / math.sqrt(D), 1 if append else 0, _lib.stream())
    ws = ws.view(B * H, n_split, 4 + D)
    return out, torch.cat([ws[..., :2], ws[..., 4:]], dim=-1)  # (m, l, o[64]): without the two pad words


def _check(B, P, offs, append):
    """offs: one offset (a shared position) or B (one per row)."""
    from nanosandbox_amd import ops

    pk, pv, kc0, vc0 = _caches(B)
    g = torch.Generator(device=DEV).manual_seed(7 * P + 13 * B + sum(offs))
    qkv = torch.randn(B, 1, 3 * H * D, device=DEV, generator=g).to(BF)
    q, kn, vn = qkv.view(B, 3, H, D).unbind(1)
    pos = torch.tensor([P + o for o in offs], device=DEV, dtype=torch.int64)
    rows = offs if len(offs) > 1 else offs * B
    # what the caches hold after the append
    kc1, vc1 = kc0.clone(), vc0.clone()
    for b, o in enumerate(rows):
        kc1[b, :, o], vc1[b, :, o] = kn[b], vn[b]
    kc, vc = (kc0.clone(), vc0.clone()) if append else (kc1.clone(), vc1.clone())
    pkc, pvc = pk.clone(), pv.clone()
    out, ws = _run_shared(qkv, pkc, pvc, kc, vc, P, pos, append)
    torch.cuda.synchronize()
    assert torch.equal(pkc, pk) and torch.equal(pvc, pv)      # the prompt caches are never written
    assert torch.equal(kc, kc1) and torch.equal(vc, vc1)      # the new rows at slot pos - P, bitwise; nothing else
    assert not bool(out.isnan().any()) and not bool(ws.isnan().any())  # every partial written, live or empty
    npc = -(-TP // 128)
    live = -(-P // 128)
    assert bool((ws[:, live:npc, 0] == -float("inf")).all()) and bool((ws[:, live:npc, 1:] == 0).all())
    assert bool(ws[:, :live, 0].isfinite().all())
    # (a) fp32 over the concatenated keys; (b) the unshared kernel on materialised caches
    ref = torch.empty(B, H, D, device=DEV)
    for b, o in enumerate(rows):
        k = torch.cat([pk[0, :, :P], kc1[b, :, :o + 1]], dim=1).float()
        v = torch.cat([pv[0, :, :P], vc1[b, :, :o + 1]], dim=1).float()
        att = torch.softmax(torch.einsum("hd,hkd->hk", q[b].float(), k) / math.sqrt(D), dim=-1)
        ref[b] = torch.einsum("hk,hkd->hd", att, v)
    fk = torch.cat([pk[:, :, :P].expand(B, -1, -1, -1), kc1], dim=2).contiguous()
    fv = torch.cat([pv[:, :, :P].expand(B, -1, -1, -1), vc1], dim=2).contiguous()
    un = ops.decode_attention(qkv, fk, fv, pos, H).float().view(B, H, D)
    y = out.float().view(B, H, D)
    err = ((y - ref).norm() / ref.norm()).item()
    err_un = ((un - ref).norm() / ref.norm()).item()
    print(f"B {B} P {P} offs {offs[:4]} append {append}: shared {err:.3e} unshared {err_un:.3e}")
    assert err < 1e-2, (err, err_un)
    assert err <= 2 * err_un, f"shared kernel {err:.3e} against the unshared kernel's {err_un:.3e}"
    return out


@pytest.mark.parametrize("B", [2, 3, 16, 17])
@pytest.mark.parametrize("P", [1, 37, 255, 256, 257, 700])
def test_shared_attention_kernel(kernels, P, B):
    """Partial 16-row groups and more than one group; prompt lengths around the chunk edges and
    in the last, partial chunk of the prompt cache; every row offset as a shared position, and
    unequal per-row positions."""
    for o in OFFS:
        _check(B, P, [o], append=True)
    _check(B, P, [OFFS[(b + P) % 4] for b in range(B)], append=True)
    _check(B, P, [OFFS[(b + 1) % 4] for b in range(B)], append=False)
    _check(B, P, [5], append=False)


def test_shared_attention_kernel_batch_64(kernels):
    from nanosandbox_amd import ops

    B, P = 64, 257
    offs = [OFFS[b % 4] + (b % 3) for b in range(B)]
    out = _check(B, P, offs, append=True)
    _check(B, P, [255], append=True)
    # the op is that launch
    pk, pv, kc0, vc0 = _caches(B)
    g = torch.Generator(device=DEV).manual_seed(7 * P + 13 * B + sum(offs))
    qkv = torch.randn(B, 1, 3 * H * D, device=DEV, generator=g).to(BF)
    pos = torch.tensor([P + o for o in offs], device=DEV, dtype=torch.int64)
    y = ops.decode_attention_shared(qkv, pk.clone(), pv.clone(), kc0.clone(), vc0.clone(),
                                    torch.tensor([P], device=DEV), pos, H, append=True)
    assert torch.equal(y, out)


def test_shared_attention_row_past_its_cache(kernels):
    """A slot >= R stores nothing and leaves empty row partials: the row attends over the prompt."""
    B, P = 3, 37
    pk, pv, kc0, vc0 = _caches(B)
    qkv = torch.randn(B, 1, 3 * H * D, device=DEV).to(BF)
    pos = torch.tensor([P + R, P + 3, P + R + 9], device=DEV, dtype=torch.int64)
    kc, vc = kc0.clone(), vc0.clone()
    out, ws = _run_shared(qkv, pk.clone(), pv.clone(), kc, vc, P, pos, True)
    assert not bool(out.isnan().any()) and not bool(ws.isnan().any())
    assert torch.equal(kc[0], kc0[0]) and torch.equal(kc[2], kc0[2]) and not torch.equal(kc[1], kc0[1])
    q = qkv.view(B, 3, H, D)[:, 0].float()
    for b in (0, 2):
        att = torch.softmax(torch.einsum("hd,hkd->hk", q[b], pk[0, :, :P].float()) / 8.0, dim=-1)
        ref = torch.einsum("hk,hkd->hd", att, pv[0, :, :P].float())
        assert ((out[b, 0].float().view(H, D) - ref).norm() / ref.norm()).item() < 1e-2


@pytest.mark.parametrize("per_row", [False, True])
def test_shared_graph_decode_matches_full_forward(kernels, per_row):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    B, T0, T = 4, 40, 72
    prompt = torch.randint(0, 512, (T0,), device=DEV)
    idx = torch.cat([prompt[None].expand(B, -1), torch.randint(0, 512, (B, T - T0), device=DEV)], dim=1)
    with torch.no_grad():
        full = m.forward_logits(idx)
    dg = Decoder(m, B, use_graph=True, per_row=per_row, shared_prompt=True, max_new=T - T0)
    de = Decoder(m, B, use_graph=False, per_row=per_row, shared_prompt=True, max_new=T - T0)
    try:
        with torch.no_grad():
            lg, le = dg.prefill_shared(prompt), de.prefill_shared(prompt)
            assert lg.shape == (B, 512) and torch.equal(lg, le)
            assert ((lg - full[:, T0 - 1]).norm() / full[:, T0 - 1].norm()).item() < 2e-2
            for t in range(T0, T):
                lg = dg.step(idx[:, t]).clone()
                le = de.step(idx[:, t])
                assert torch.equal(lg, le), t  # the replayed graph runs exactly the eager kernels
                err = ((lg - full[:, t]).norm() / full[:, t].norm()).item()
                assert err < 3e-2, (t, err)
        assert dg.replays == T - T0 and dg.positions == [T] * B and de.positions == [T] * B
        assert int(dg.plen) == T0 and dg.prefills == 1
    finally:
        dg.release()
        de.release()


def test_one_graph_for_two_prompt_lengths(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    B, n_new = 3, 24
    dec = Decoder(m, B, use_graph=True, per_row=True, shared_prompt=True, max_new=n_new)
    try:
        for n in (16, 90):
            p = torch.randint(0, 512, (n,), device=DEV)
            got = m.generate_batch([p] * B, n_new, top_k=1, shared_prompt=True, decoder=dec)
            want = m.generate_batch([p] * B, n_new, top_k=1, shared_prompt=True, use_graph=False)
            assert int(dec.plen) == n and dec.positions == [n + n_new - 1] * B
            for u, v in zip(got, want):
                assert u.numel() == n + n_new and torch.equal(u, v) and torch.equal(u[:n], p)
        assert len(dec.sgraphs) == 1 and dec.prefills == 2  # the graph is not keyed by the prompt length
    finally:
        dec.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_shared_batch_sampling_and_stop_token(kernels):
    m = _model()
    B, n_new = 5, 40
    p = torch.randint(0, 512, (11,), device=DEV)
    torch.manual_seed(7)
    free = m.generate_batch([p] * B, n_new, temperature=1.0, shared_prompt=True)
    assert all(y.numel() == 11 + n_new and torch.equal(y[:11], p) for y in free)
    assert not all(torch.equal(free[0], y) for y in free[1:])  # the rows draw independently
    stop = int(free[0][11 + 6])
    torch.manual_seed(7)  # the same salts: the same draws, now cut at the stop token
    ys = m.generate_batch([p] * B, n_new, temperature=1.0, shared_prompt=True, stop_token=stop)
    for y, f in zip(ys, free):
        new, fnew = y[11:], f[11:].tolist()
        assert torch.equal(y[:11], p) and 1 <= new.numel() <= n_new
        assert int(new.min()) >= 0 and int(new.max()) < 512
        cut = fnew[:fnew.index(stop) + 1] if stop in fnew else fnew
        assert new.tolist() == cut
    assert int(ys[0][-1]) == stop and ys[0].numel() <= 11 + 7
    assert not all(torch.equal(ys[0], y) for y in ys[1:])
    assert not [n for n, prm in m.named_parameters() if hasattr(prm, "compute")]


def _dequantized_copy(m):  # tests/test_quant_gpu.py's
    from nanosandbox_amd import ops

    m2 = copy.deepcopy(m)
    ps = [m2.lm_head.weight]
    for blk in m2.transformer.h:
        ps += [blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight]
    with torch.no_grad():
        for p in ps:
            p.copy_(ops.dequantize(ops.quantize_rows_int8(p)))
    return m2


def test_shared_decoder_with_int8_weights(kernels):
    """The int8 tests' bounds (tests/test_quant_gpu.py: 2e-2 after the prompt, 3e-2 per step,
    against the model holding the dequantized weights), here against the unquantized shared
    decoder of that model."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    m2 = _dequantized_copy(m)
    B, T0, n_new = 4, 40, 16
    prompt = torch.randint(0, 512, (T0,), device=DEV)
    toks = torch.randint(0, 512, (B, n_new), device=DEV)
    dq = Decoder(m, B, use_graph=True, per_row=True, quantize="int8", shared_prompt=True, max_new=n_new)
    d0 = Decoder(m2, B, use_graph=False, per_row=True, shared_prompt=True, max_new=n_new)
    try:
        with torch.no_grad():
            a, b = dq.prefill_shared(prompt), d0.prefill_shared(prompt)
            assert ((a - b).norm() / b.norm()).item() < 2e-2
            for t in range(n_new):
                a, b = dq.step(toks[:, t]), d0.step(toks[:, t])
                err = ((a - b).norm() / b.norm()).item()
                assert err < 3e-2, (t, err)
        ys = m.generate_batch([prompt] * B, n_new, temperature=1.0, shared_prompt=True, quantize="int8", decoder=dq)
        assert dq.prefills == 1 and all(y.numel() == T0 + n_new and torch.equal(y[:T0], prompt) for y in ys)
    finally:
        dq.release()
        d0.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
