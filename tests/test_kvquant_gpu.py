"""int8 KV caches on gfx950: the ``_kv8`` append and attention kernels (csrc/kernels/decode.hip)
and ``Decoder(kv_quantize="int8")``.  The quantizer reference is ``ops.quantize_cache_rows`` run
on the CPU from the same bf16 values (bit equality: bytes and scales); the attention reference
is fp32 torch over ``ops.dequantize_cache``."""

import copy
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
D = 64


def _record(monkeypatch):
    from nanosandbox_amd.ops import functional

    calls = []
    real_call = functional._lib.call
    monkeypatch.setattr(functional._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    return calls


def _to(qc, dev):
    from nanosandbox_amd import ops

    return ops.QuantCache(qc.q.to(dev).clone(), qc.scale.to(dev).clone())


def _same(a, b):
    return torch.equal(a.q.cpu(), b.q.cpu()) and torch.equal(a.scale.cpu(), b.scale.cpu())


def _random_cache(B, H, T, seed):
    """CPU QuantCache: any byte in +-127, scales in [0.004, 0.02] (values up to ~2.5)."""
    from nanosandbox_amd import ops

    g = torch.Generator().manual_seed(seed)
    q = torch.randint(-127, 128, (B, H, T, D), generator=g, dtype=torch.int32).to(torch.int8)
    return ops.QuantCache(q, torch.rand(B, H, T, generator=g) * 0.016 + 0.004)


def _kv_rows(qkv, H):
    """K and V rows of a decode-step qkv [B, 1, 3C] on the CPU: [B, H, D] each (fp32 values of the bf16)."""
    x = qkv.detach().cpu().float().view(qkv.shape[0], 3, H, D)
    return x[:, 1], x[:, 2]


# ---------------------------------------------------------------------------- 5. prefill append

@pytest.mark.parametrize("pos", [None, 0, 20, 100])  # host 0; device position; 100: rows past Tmax are dropped
def test_kv8_prefill_append(kernels, monkeypatch, pos):
    from nanosandbox_amd import ops

    B, S, H, T = 2, 77, 4, 128
    C = H * D
    torch.manual_seed(S + (pos or 0))
    qkv = (torch.randn(B, S, 3 * C) * torch.logspace(-3, 2, S).view(1, S, 1)).to(BF)
    qkv[0, 5, C:C + D] = 0.0          # an all-zero K row (head 0)
    qkv[1, 7, 2 * C + D:2 * C + 2 * D] = -0.75  # a constant V row (head 1)
    p0 = pos or 0
    n = min(S, T - p0)
    want = []
    for i in (1, 2):
        rows = qkv.float().view(B, S, 3, H, D)[:, :n, i].transpose(1, 2)  # [B, H, n, D]
        qc = ops.quantize_cache_rows(rows)  # on the CPU
        full = ops.QuantCache(torch.zeros(B, H, T, D, dtype=torch.int8), torch.ones(B, H, T))
        full.q[:, :, p0:p0 + n] = qc.q
        full.scale[:, :, p0:p0 + n] = qc.scale
        want.append(full)
    kc = ops.QuantCache(torch.zeros(B, H, T, D, dtype=torch.int8, device=DEV), torch.ones(B, H, T, device=DEV))
    vc = ops.QuantCache(torch.zeros(B, H, T, D, dtype=torch.int8, device=DEV), torch.ones(B, H, T, device=DEV))
    calls = _record(monkeypatch)
    if pos is None:
        ops.kv_append(qkv.to(DEV), kc, vc, None, 0)
    else:
        ops.kv_append(qkv.to(DEV), kc, vc, torch.tensor([pos], device=DEV, dtype=torch.int64))
    assert calls == ["nsa_kv_append_kv8"]
    assert torch.equal(kc.q.cpu(), want[0].q) and torch.equal(kc.scale.cpu(), want[0].scale)
    assert torch.equal(vc.q.cpu(), want[1].q) and torch.equal(vc.scale.cpu(), want[1].scale)
    assert float(kc.scale[0, 0, p0 + 5]) == 1.0 and bool((vc.q[1, 1, p0 + 7] == -127).all())


# ---------------------------------------------------------------------------- 6. attention kernel

def _attn_ref(qkv, kc, vc, positions, H):
    """fp32 torch over the dequantized caches (CPU): [B, H * D]."""
    from nanosandbox_amd import ops

    B = qkv.shape[0]
    q = qkv.detach().cpu().float().view(B, 3, H, D)[:, 0]
    kd, vd = ops.dequantize_cache(_to(kc, "cpu")), ops.dequantize_cache(_to(vc, "cpu"))
    out = torch.empty(B, H, D)
    for b, p in enumerate(positions):
        att = torch.softmax(torch.einsum("hd,hkd->hk", q[b], kd[b, :, :p + 1]) / math.sqrt(D), dim=-1)
        out[b] = torch.einsum("hk,hkd->hd", att, vd[b, :, :p + 1])
    return out.view(B, H * D)


ATTN_CASES = [pytest.param(1024, [p], id=str(p)) for p in (0, 37, 255, 256, 700, 1023)]
ATTN_CASES += [pytest.param(1024, [0, 255, 256], id="rows"), pytest.param(300, [299], id="T300")]


@pytest.mark.parametrize("T,positions", ATTN_CASES)
def test_kv8_attention_kernel(kernels, monkeypatch, T, positions):
    from nanosandbox_amd import ops

    B, H = 3, 12
    C = H * D
    torch.manual_seed(T + sum(positions))
    k0, v0 = _random_cache(B, H, T, 1), _random_cache(B, H, T, 2)
    qkv = torch.randn(B, 1, 3 * C).to(BF).to(DEV)
    pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
    plist = positions if len(positions) == B else positions * B
    k1, v1, k2, v2 = _to(k0, DEV), _to(v0, DEV), _to(k0, DEV), _to(v0, DEV)
    calls = _record(monkeypatch)
    y1 = ops.decode_attention(qkv, k1, v1, pos, H, append=True)
    assert calls == ["nsa_decode_attn_rows_kv8" if len(positions) > 1 else "nsa_decode_attn_kv8"]
    assert y1.shape == (B, 1, C) and y1.dtype == BF
    # the appended rows are the CPU quantizer's, and nothing else moved
    kn, vn = _kv_rows(qkv, H)
    kw, vw = _to(k0, "cpu"), _to(v0, "cpu")
    for b, p in enumerate(plist):
        for new, c in ((kn, kw), (vn, vw)):
            qc = ops.quantize_cache_rows(new[b])
            c.q[b, :, p], c.scale[b, :, p] = qc.q, qc.scale
    assert _same(k1, kw) and _same(v1, vw)
    ref = _attn_ref(qkv, k1, v1, plist, H)
    err = ((y1.float().cpu().view(B, C) - ref).norm() / ref.norm()).item()
    assert err < 1e-2, err
    # append=True == kv_append, then append=False: bit for bit
    ops.kv_append(qkv, k2, v2, pos)
    assert _same(k2, kw) and _same(v2, vw)
    y2 = ops.decode_attention(qkv, k2, v2, pos, H, append=False)
    assert torch.equal(y1, y2)
    assert _same(k2, kw) and _same(v2, vw)


# ---------------------------------------------------------------------------- 7. exact V pin

@pytest.mark.parametrize("pos", [0, 300, 1023])
def test_kv8_exact_v_pin(kernels, pos):
    """q = 0: every score is 0, so each chunk's partial is m = 0, l = its live keys and o = the
    plain sum of its dequantized V rows.  Bytes times power-of-two scales 2^-3 .. 2^2: every
    partial sum is a multiple of 2^-3 below 2^24 (256 keys * 127 * 4 * 8 < 2^21), so fp32 is exact
    in any order and o must equal the float64 sum bit for bit."""
    from nanosandbox_amd import ops

    H, T = 2, 1024
    C = H * D
    torch.manual_seed(pos)
    kc = _random_cache(1, H, T, 3)
    vq = torch.randint(-127, 128, (1, H, T, D), dtype=torch.int32).to(torch.int8)
    vq[..., 0], vq[..., 63] = 127, -127
    vs = torch.pow(2.0, ((torch.arange(T) + torch.arange(H).view(H, 1)) % 6 - 3).float()).view(1, H, T)
    vc = ops.QuantCache(vq, vs.contiguous())
    qkv = torch.randn(1, 1, 3 * C).to(BF)
    qkv[..., :C] = 0.0
    part = ops.decode_attention(qkv.to(DEV), _to(kc, DEV), _to(vc, DEV),
                                torch.tensor([pos], device=DEV, dtype=torch.int64), H, append=False, combine=False)
    assert isinstance(part, ops.AttnPartials) and part.n_split == 4
    ws = part.ws.cpu().view(H, 4, 4 + D)
    deq = (vq.double() * vs.double()[..., None])[0]  # [H, T, D]
    for s in range(4):
        lo, hi = 256 * s, min(256 * s + 255, pos)
        if lo > pos:  # empty partial
            assert bool((ws[:, s, 0] == -math.inf).all()) and bool((ws[:, s, 1] == 0).all())
            assert bool((ws[:, s, 4:] == 0).all())
            continue
        assert bool((ws[:, s, 0] == 0).all()) and bool((ws[:, s, 1] == hi - lo + 1).all()), (s, ws[:, s, :2])
        want = deq[:, lo:hi + 1].sum(dim=1)
        assert torch.equal(want.float().double(), want)
        assert torch.equal(ws[:, s, 4:], want.float()), s


# ---------------------------------------------------------------------------- 8. exact K pin

@pytest.mark.parametrize("pos", [0, 300, 1023])
def test_kv8_exact_k_pin(kernels, pos):
    """q = +-1; the target key of each (b, h) is 127 sign(q) with scale 1: score 127 * 64 / 8 =
    1016; every other key is -(0..127) sign(q) times a power of two: score <= 0, weight
    2^(-1016 * log2 e) = 0 in fp32.  The output is the target's dequantized V row, a byte times a
    power of two: exact in bf16.  Append form: the new token's K / V rows go through the
    in-kernel quantizer (the V row holds +-127, so its scale is the power of two itself)."""
    from nanosandbox_amd import ops

    B, H, T = 2, 3, 1024
    C = H * D
    torch.manual_seed(pos + 1)
    sign = (torch.randint(0, 2, (B, H, D)) * 2 - 1).float()
    target = torch.randint(0, pos + 1, (B, H))
    target[0, 0] = pos           # the appended row itself
    target[1, 2] = 0 if pos else pos
    pw = lambda *shape: torch.pow(2.0, torch.randint(-3, 3, shape).float())  # noqa: E731
    kq = -torch.randint(0, 128, (B, H, T, D)).float() * sign.view(B, H, 1, D)
    ks = pw(B, H, T)
    vq = torch.randint(-127, 128, (B, H, T, D)).float()
    vq[..., 0], vq[..., 63] = -127, 127
    vs = pw(B, H, T)
    for b in range(B):
        for h in range(H):
            kq[b, h, target[b, h]] = 127 * sign[b, h]
            ks[b, h, target[b, h]] = 1.0
    # the new token: q, and the K / V rows of position pos as bf16 values (exact: 7-bit integers
    # times powers of two)
    qkv = torch.stack([sign, kq[:, :, pos] * ks[:, :, pos, None], vq[:, :, pos] * vs[:, :, pos, None]], dim=1)
    assert torch.equal(qkv.to(BF).float(), qkv)
    want = (vq * vs[..., None])[torch.arange(B).view(B, 1), torch.arange(H).view(1, H), target]  # [B, H, D]
    # the cache rows at pos start as junk: the kernel must take them from the new token
    kq[:, :, pos], vq[:, :, pos] = 99.0, 99.0
    kc = ops.QuantCache(kq.to(torch.int8).to(DEV), ks.to(DEV).contiguous())
    vc = ops.QuantCache(vq.to(torch.int8).to(DEV), vs.to(DEV).contiguous())
    for per_row in (False, True):
        p = torch.full((B if per_row else 1,), pos, device=DEV, dtype=torch.int64)
        k1, v1 = _to(kc, DEV), _to(vc, DEV)
        y = ops.decode_attention(qkv.view(B, 1, 3 * C).to(BF).to(DEV), k1, v1, p, H, append=True)
        assert torch.equal(y.cpu().view(B, H, D), want.to(BF)), per_row
        assert torch.equal(v1.scale[:, :, pos].cpu(), vs[:, :, pos])  # +-127 present: the scale itself


# ---------------------------------------------------------------------------- 9. decoder

def _model_cpu():  # tests/test_quant_gpu.py's, before the move to the GPU
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0,
                         bias=False)).eval()


def _model():
    return _model_cpu().to(DEV).set_compute_dtype(BF)


def _dequantized_copy(m):
    """A deep copy whose quantized weight groups hold dequantize(quantize_rows_int8(w))."""
    from nanosandbox_amd import ops

    m2 = copy.deepcopy(m)
    ps = [m2.lm_head.weight]
    for blk in m2.transformer.h:
        ps += [blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight]
    with torch.no_grad():
        for p in ps:
            p.copy_(ops.dequantize(ops.quantize_rows_int8(p)))
    return m2


def _e_q(m_cpu, idx, T0):
    """The int8 caches' own error for this batch: the CPU fp32 reference path (no kernel) against
    the same fp32 model's full forward, max over the steps of the relative Frobenius error."""
    from nanosandbox_amd.runtime.decode import Decoder

    idx = idx.cpu()
    with torch.no_grad():
        full = m_cpu.forward_logits(idx)
        dec = Decoder(m_cpu, idx.shape[0], use_graph=False, kv_quantize="int8")
        dec.prefill(idx[:, :T0])
        worst = 0.0
        for t in range(T0, idx.shape[1]):
            lg = dec.step(idx[:, t])
            worst = max(worst, ((lg - full[:, t]).norm() / full[:, t].norm()).item())
        dec.release()
    return worst


@pytest.mark.parametrize("B,quantize", [(1, None), (4, None), (12, None), (20, None),
                                        (1, "int8"), (4, "int8"), (12, "int8")])
def test_kv8_graph_decode(kernels, monkeypatch, B, quantize):
    """The kv8 graph step equals the kv8 eager step bit for bit, and follows the full forward of
    the model (with ``quantize``: of its dequantized-weight copy) within 3e-2 + 2 E_q: 3e-2 is the
    bound of the bf16 step, E_q the int8 caches' own error measured on the CPU in fp32, doubled
    because a bf16-rounded K / V value can land on the other side of a rounding boundary.
    B = 20 is past the int8-weight row cap: the caches have none."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    m2 = _dequantized_copy(m) if quantize else m
    m_cpu = _dequantized_copy(_model_cpu()) if quantize else _model_cpu()
    T0, T = 40, 72
    torch.manual_seed(0)
    idx = torch.randint(0, 512, (B, T), device=DEV)
    e_q = _e_q(m_cpu, idx, T0)
    assert 0 < e_q < 1e-2, e_q
    bound = 3e-2 + 2 * e_q
    with torch.no_grad():
        full = m2.forward_logits(idx)
    dg = Decoder(m, B, use_graph=True, quantize=quantize, kv_quantize="int8")
    de = Decoder(m, B, use_graph=False, quantize=quantize, kv_quantize="int8")
    try:
        worst = 0.0
        with torch.no_grad():
            lg, le = dg.prefill(idx[:, :T0]), de.prefill(idx[:, :T0])
            ref = full[:, T0 - 1]
            assert ((lg - ref).norm() / ref.norm()).item() < 2e-2  # the prompt's attention is unquantized
            for t in range(T0, T):
                lg = dg.step(idx[:, t]).clone()
                le = de.step(idx[:, t])
                assert torch.equal(lg, le), t
                err = ((lg - full[:, t]).norm() / full[:, t].norm()).item()
                worst = max(worst, err)
                assert err < bound, (t, err, e_q)
        print(f"B={B} quantize={quantize}: E_q={e_q:.3e} worst={worst:.3e} bound={bound:.3e}")
        assert dg.replays == T - T0 and dg.position == T
        if B == 1:
            # one more eager step: as many launches as the bf16-cache decoder's, the attention
            # kernel's kv8 form once per layer and no bf16-cache kernel
            calls = _record(monkeypatch)
            with torch.no_grad():
                de.step(idx[:, 0])
                nq = list(calls)
                d0 = Decoder(m, 1, use_graph=False, quantize=quantize)
                d0.prefill(idx[:, :T0])
                del calls[:]
                d0.step(idx[:, T0])
                n0 = list(calls)
                d0.release()
            assert len(nq) == len(n0), (nq, n0)
            assert nq.count("nsa_decode_attn_kv8") == 3 and n0.count("nsa_decode_attn") == 3
            assert not [c for c in nq if c in ("nsa_decode_attn", "nsa_decode_attn_rows", "nsa_kv_append")], nq
    finally:
        de.release()
        dg.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_kv8_per_row_graph_decode(kernels):
    """per_row decoders with unequal prompts: graph == eager bit for bit, and each row follows
    the full forward of its own sequence within the same bound."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    lens = [40, 17, 33, 5]
    B, n_new = len(lens), 24
    torch.manual_seed(2)
    idx = torch.randint(0, 512, (B, max(lens) + n_new), device=DEV)
    e_q = _e_q(_model_cpu(), idx[:, :40 + n_new], 40)
    with torch.no_grad():
        full = [m.forward_logits(idx[b:b + 1, :lens[b] + n_new])[0] for b in range(B)]
    dg = Decoder(m, B, use_graph=True, per_row=True, kv_quantize="int8")
    de = Decoder(m, B, use_graph=False, per_row=True, kv_quantize="int8")
    try:
        with torch.no_grad():
            L = torch.tensor(lens, device=DEV)
            dg.prefill(idx[:, :max(lens)], L)
            de.prefill(idx[:, :max(lens)], L)
            for t in range(n_new):
                tok = torch.stack([idx[b, lens[b] + t] for b in range(B)])
                lg = dg.step(tok).clone()
                assert torch.equal(lg, de.step(tok)), t
                for b in range(B):
                    ref = full[b][lens[b] + t]
                    err = ((lg[b] - ref).norm() / ref.norm()).item()
                    assert err < 3e-2 + 2 * e_q, (t, b, err)
        assert dg.positions == [n + n_new for n in lens]
    finally:
        de.release()
        dg.release()


def test_kv8_decoder_refuses_models_without_kernels(kernels):
    from nanosandbox_amd.models import GPT, GPTConfig
    from nanosandbox_amd.runtime.decode import Decoder

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=64, vocab_size=128, n_layer=1, n_head=4, n_embd=128, dropout=0.0, bias=False))
    m = m.eval().to(DEV).set_compute_dtype(BF)  # head_dim 32
    with pytest.raises(ValueError):
        Decoder(m, 2, kv_quantize="int8")
    with pytest.raises(ValueError):
        Decoder(_model(), 2, kv_quantize="fp8")
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


# ---------------------------------------------------------------------------- 10. front ends

@pytest.mark.parametrize("quantize", [None, "int8"])
def test_kv8_front_ends_on_gpu(kernels, quantize):
    """Greedy (top_k=1) generation, graph against eager, token for token.  Every call starts
    from the same torch seed, so the decoders draw the same sampling stream: the prompt's
    logits are bf16-rounded, where two tokens can tie for the maximum, and a tie is broken by
    the stream."""
    m = _model()
    kw = dict(top_k=1, kv_quantize="int8", quantize=quantize)

    def run(fn, *a, **k):
        torch.manual_seed(11)
        return fn(*a, **k, **kw)

    g = torch.Generator().manual_seed(4)  # host RNG: the same prompts everywhere
    idx = torch.randint(0, 512, (2, 8), generator=g).to(DEV)
    a = run(m.generate_cached, idx, 40, use_graph=True)
    b = run(m.generate_cached, idx, 40, use_graph=False)
    assert a.shape == (2, 48) and torch.equal(a, b) and torch.equal(a[:, :8], idx)

    prompts = [torch.randint(0, 512, (n,), generator=g).to(DEV) for n in (3, 5, 9)]
    free = run(m.generate_batch, prompts, 24, use_graph=False)
    stop = int(free[0][3 + 6])  # row 0 draws it as its 7th new token at the latest
    ya = run(m.generate_batch, prompts, 24, stop_token=stop, use_graph=True)
    yb = run(m.generate_batch, prompts, 24, stop_token=stop, use_graph=False)
    for p, u, v in zip(prompts, ya, yb):
        assert torch.equal(u, v) and torch.equal(u[:p.numel()], p)
        new = u[p.numel():]
        assert 1 <= new.numel() <= 24 and int(new.min()) >= 0 and int(new.max()) < 512
        assert new.numel() == 24 or int(new[-1]) == stop
        assert stop not in new[:-1].tolist()
    assert int(ya[0][-1]) == stop and ya[0].numel() <= 3 + 7
    with pytest.raises(ValueError):  # a row that would fall to the recompute loop
        m.generate_batch([prompts[0], torch.zeros(250, dtype=torch.int64, device=DEV)], 24, **kw)
    with pytest.raises(ValueError):
        m.generate_cached(idx, 250, **kw)
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
