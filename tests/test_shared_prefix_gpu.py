"""A shared prompt prefix on MI355X: the prefix-attention kernel against an fp32 reference and
against the flash forward on the materialised sequences, ``Decoder.prefill_suffixes`` and the
steps after it against the full fused forward, one captured graph for two prefixes, and the
batch front end with sampling, stop tokens and int8 weights."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
H, D, TP = 4, 64, 320
C = H * D
PS = [1, 31, 32, 33, 128, 300]        # prefix lengths: one key, around a wave's 32 keys, a full round, several
SS = [1, 15, 16, 17, 64, 65, 130]     # suffix lengths: around the 16-query tile, several tiles, a partial last one


def _model():  # tests/test_shared_prompt_gpu.py's
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


def _bits(t):
    return t.view(torch.int16)


def _rel(y, ref):
    """(whole-tensor relative error, the worst query row's relative error); y, ref: [B, S, C]."""
    rows = (y - ref).norm(dim=-1) / ref.norm(dim=-1)
    return ((y - ref).norm() / ref.norm()).item(), rows.max().item()


def _check(B, P, S):
    from nanosandbox_amd import ops
    from nanosandbox_amd.ops import _lib

    g = torch.Generator(device=DEV).manual_seed(1000 * P + 10 * S + B)
    full = torch.randn(B, P + S, 3 * C, device=DEV, generator=g).to(BF)
    full[:, :P] = full[:1, :P].clone()  # one prefix for every row
    qf, kf, vf = full.float().view(B, P + S, 3, H, D).permute(2, 0, 3, 1, 4)  # [B, H, P + S, D]
    pk = torch.full((1, H, TP, D), float("nan"), device=DEV, dtype=BF)  # rows >= P: NaN, never to be used
    pv = pk.clone()
    pk[0, :, :P], pv[0, :, :P] = kf[0, :, :P].to(BF), vf[0, :, :P].to(BF)
    qkv = full[:, P:].contiguous()
    out = torch.full((B, S, C), float("nan"), device=DEV, dtype=BF)
    q0, pk0, pv0 = qkv.clone(), pk.clone(), pv.clone()
    _lib.call("nsa_prefix_attn", _lib.ptr(qkv), _lib.ptr(pk), _lib.ptr(pv), _lib.ptr(out), B, S, H, TP, P,
              1.0 / math.sqrt(D), _lib.stream())
    torch.cuda.synchronize()
    assert not bool(out.isnan().any()), (B, P, S)  # every row written, none touched by a dead cache row
    assert torch.equal(_bits(qkv), _bits(q0)) and torch.equal(_bits(pk), _bits(pk0)) and torch.equal(_bits(pv), _bits(pv0))
    assert torch.equal(ops.prefix_attention(qkv, pk, pv, P, H), out)  # the op is that launch
    # (a) fp32 causal attention over the whole sequence, outputs at P ..; (b) the flash forward on it
    att = (qf @ kf.transpose(-2, -1)) / math.sqrt(D)
    mask = torch.ones(P + S, P + S, dtype=torch.bool, device=DEV).tril()
    ref = (torch.softmax(att.masked_fill(~mask, float("-inf")), dim=-1) @ vf).transpose(1, 2).reshape(B, P + S, C)[:, P:]
    fl = ops.attention(full, H, 0.0, False)[:, P:].float()
    err, row = _rel(out.float(), ref)
    err_fl, row_fl = _rel(fl, ref)
    print(f"B {B} P {P} S {S}: prefix kernel {err:.3e} (worst row {row:.3e}) flash {err_fl:.3e} (worst row {row_fl:.3e})")
    assert err < 1e-2, (err, err_fl)
    assert err <= 2 * err_fl, f"prefix kernel {err:.3e} against the flash kernel's {err_fl:.3e}"
    assert row <= 2 * row_fl, f"worst row: prefix kernel {row:.3e} against the flash kernel's {row_fl:.3e}"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("half", [0, 1])
def test_prefix_attention_kernel(kernels, B, half):
    for P in PS[3 * half:3 * half + 3]:
        for S in SS:
            _check(B, P, S)


def _rows(B, P, lens, n_new):
    """prefix [P], right-padded suffixes [B, S], step tokens [B, n_new] and the rows they make,
    right-padded to [B, P + S + n_new] (causality keeps the padding out of a row's own positions)."""
    S = max(lens)
    prefix = torch.randint(0, 512, (P,), device=DEV)
    suf = torch.randint(0, 512, (B, S), device=DEV)
    toks = torch.randint(0, 512, (B, n_new), device=DEV)
    idx = torch.zeros(B, P + S + n_new, dtype=torch.int64, device=DEV)
    for b, n in enumerate(lens):
        idx[b, :P + n + n_new] = torch.cat([prefix, suf[b, :n], toks[b]])
    return prefix, suf, toks, idx


def test_prefix_graph_decode_matches_full_forward(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    B, P, n_new = 4, 40, 24
    lens = [1, 5, 16, 17]
    prefix, suf, toks, idx = _rows(B, P, lens, n_new)
    lengths = torch.tensor(lens, device=DEV)
    ar = torch.arange(B, device=DEV)
    with torch.no_grad():
        full = m.forward_logits(idx)
    dg = Decoder(m, B, use_graph=True, per_row=True, shared_prompt=True, max_new=max(lens) + n_new)
    de = Decoder(m, B, use_graph=False, per_row=True, shared_prompt=True, max_new=max(lens) + n_new)
    try:
        with torch.no_grad():
            dg.prefill_shared(prefix), de.prefill_shared(prefix)
            lg, le = dg.prefill_suffixes(suf, lengths), de.prefill_suffixes(suf, lengths)
            want = full[ar, P + lengths - 1]
            assert lg.shape == (B, 512) and torch.equal(lg, le)
            assert ((lg - want).norm() / want.norm()).item() < 2e-2
            assert dg.positions == [P + n for n in lens]
            for t in range(n_new):
                lg = dg.step(toks[:, t]).clone()
                le = de.step(toks[:, t])
                assert torch.equal(lg, le), t  # the replayed graph runs exactly the eager kernels
                want = full[ar, P + lengths + t]
                err = ((lg - want).norm() / want.norm()).item()
                assert err < 3e-2, (t, err)
        assert dg.replays == n_new and dg.positions == de.positions == [P + n + n_new for n in lens]
        assert int(dg.plen) == P and dg.prefills == 1
    finally:
        dg.release()
        de.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_one_graph_for_two_prefixes(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    B, n_new = 3, 24
    dec = Decoder(m, B, use_graph=True, per_row=True, shared_prompt=True, max_new=20 + n_new)
    try:
        for n, lens in ((16, [3, 20, 1]), (90, [17, 2, 9])):
            prefix = torch.randint(0, 512, (n,), device=DEV)
            ps = [torch.cat([prefix, torch.randint(0, 512, (k,), device=DEV)]) for k in lens]
            ps[1][n] = (ps[0][n] + 1) % 512  # the common prefix is exactly n tokens
            got = m.generate_batch(ps, n_new, top_k=1, shared_prefix=True, decoder=dec)
            want = m.generate_batch(ps, n_new, top_k=1, shared_prefix=True, use_graph=False)
            assert int(dec.plen) == n and dec.positions == [n + k + n_new - 1 for k in lens]
            for p, u, v in zip(ps, got, want):
                assert u.numel() == p.numel() + n_new and torch.equal(u, v) and torch.equal(u[:p.numel()], p)
        assert len(dec.sgraphs) == 1 and dec.prefills == 2  # the graph is keyed by neither prefix nor suffixes
    finally:
        dec.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_prefix_batch_sampling_and_stop_token(kernels):
    m = _model()
    B, n_new, P = 5, 40, 11
    prefix = torch.randint(0, 512, (P,), device=DEV)
    ps = [torch.cat([prefix, torch.randint(0, 512, (k,), device=DEV)]) for k in (1, 4, 4, 9, 2)]
    ps[2] = ps[1].clone()  # two rows with one prompt still draw independently
    torch.manual_seed(7)
    free = m.generate_batch(ps, n_new, temperature=1.0, shared_prefix=True)
    assert all(y.numel() == p.numel() + n_new and torch.equal(y[:p.numel()], p) for p, y in zip(ps, free))
    assert not torch.equal(free[1], free[2])
    stop = int(free[0][ps[0].numel() + 6])
    torch.manual_seed(7)  # the same salts: the same draws, now cut at the stop token
    ys = m.generate_batch(ps, n_new, temperature=1.0, shared_prefix=True, stop_token=stop)
    for p, y, f in zip(ps, ys, free):
        n = p.numel()
        new, fnew = y[n:], f[n:].tolist()
        assert torch.equal(y[:n], p) and 1 <= new.numel() <= n_new
        assert int(new.min()) >= 0 and int(new.max()) < 512
        cut = fnew[:fnew.index(stop) + 1] if stop in fnew else fnew
        assert new.tolist() == cut
    assert int(ys[0][-1]) == stop and ys[0].numel() <= ps[0].numel() + 7
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


def test_prefix_decoder_with_int8_weights(kernels):
    """The int8 tests' bounds (tests/test_quant_gpu.py: 2e-2 after the prompt, 3e-2 per step,
    against the model holding the dequantized weights), here against the unquantized shared-prefix
    decoder of that model."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    m2 = _dequantized_copy(m)
    B, P, n_new = 4, 40, 16
    lens = [1, 5, 16, 17]
    prefix, suf, toks, idx = _rows(B, P, lens, n_new)
    lengths = torch.tensor(lens, device=DEV)
    R = max(lens) + n_new
    dq = Decoder(m, B, use_graph=True, per_row=True, quantize="int8", shared_prompt=True, max_new=R)
    d0 = Decoder(m2, B, use_graph=False, per_row=True, shared_prompt=True, max_new=R)
    try:
        with torch.no_grad():
            dq.prefill_shared(prefix), d0.prefill_shared(prefix)
            a, b = dq.prefill_suffixes(suf, lengths), d0.prefill_suffixes(suf, lengths)
            assert ((a - b).norm() / b.norm()).item() < 2e-2
            for t in range(n_new):
                a, b = dq.step(toks[:, t]), d0.step(toks[:, t])
                err = ((a - b).norm() / b.norm()).item()
                assert err < 3e-2, (t, err)
        ps = [torch.cat([prefix, suf[b, :n]]) for b, n in enumerate(lens)]
        ps[1][P] = (ps[0][P] + 1) % 512  # the common prefix is exactly P tokens
        ys = m.generate_batch(ps, n_new, temperature=1.0, shared_prefix=True, quantize="int8", decoder=dq)
        assert dq.prefills == 1 and all(y.numel() == p.numel() + n_new and torch.equal(y[:p.numel()], p)
                                        for p, y in zip(ps, ys))
    finally:
        dq.release()
        d0.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
