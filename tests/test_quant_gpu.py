"""int8 weight-only decode kernels (csrc/kernels/decode_q8.hip) and the quantized Decoder on
gfx950.  The reference of every kernel test is fp32 torch on ``ops.dequantize(qw)`` with the
activations bf16-rounded as tests/test_decode_gpu.py does; tolerance: its relative
Frobenius error < 1e-2 for the same kernels."""

import copy

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16

BF16_STREAM = {"nsa_gemv", "nsa_gemv_ln", "nsa_gemv_emb_ln", "nsa_gemv_attn", "nsa_skinny_gemm",
               "nsa_skinny_ln_gemm"}
Q8_STREAM = {n + "_q8" for n in BF16_STREAM}


def _record(monkeypatch):
    from nanosandbox_amd.ops import functional

    calls = []
    real_call = functional._lib.call
    monkeypatch.setattr(functional._lib, "call", lambda name, *a: (calls.append(name), real_call(name, *a))[1])
    return calls


def _only_q8(calls, expected):
    """``expected`` ran, and neither a bf16 weight stream nor a GEMM of the dequantize fallback."""
    assert expected in calls, calls
    assert not [c for c in calls if c in BF16_STREAM or c.startswith("nsa_gemm")], calls


def _weights(N, K, bias, seed):
    from nanosandbox_amd import ops

    torch.manual_seed(seed)
    w = torch.randn(N, K, device=DEV) * 0.05
    qw = ops.quantize_rows_int8(w)
    b = (torch.randn(N, device=DEV) * 0.1).to(BF) if bias else None
    return qw, ops.dequantize(qw), b


def _ref(h, dq, b, gelu):
    ref = h @ dq.t()
    if b is not None:
        ref = ref + b.float()
    return F.gelu(ref) if gelu else ref


def _relerr(y, ref):
    return ((y.float().reshape(ref.shape) - ref).norm() / ref.norm()).item()


ROW_SHAPES = [(768, 768, True, False, False), (3072, 768, True, True, False), (768, 3072, False, False, False),
              (50304, 768, False, False, True), (4800, 1600, True, False, False),
              (100, 64, True, True, False),      # N tail and a single K piece
              (50257, 768, False, False, True)]  # odd N


@pytest.mark.parametrize("N,K,bias,gelu,f32", ROW_SHAPES)
def test_q8_single_row_kernels(kernels, monkeypatch, N, K, bias, gelu, f32):
    """nsa_gemv_q8 and nsa_gemv_ln_q8 (with and without a branch, s checked, pos_inc once)."""
    from nanosandbox_amd import ops

    calls = _record(monkeypatch)
    qw, dq, b = _weights(N, K, bias, N + K)
    x = torch.randn(1, 1, K, device=DEV).to(BF)
    y = ops.decode_linear(x, qw, b, gelu=gelu, out_f32=f32)
    _only_q8(calls, "nsa_gemv_q8")
    assert y.shape == (1, 1, N) and y.dtype == (torch.float32 if f32 else BF)
    err = _relerr(y, _ref(x.float().view(1, K), dq, b, gelu))
    assert err < 1e-2, err

    lw = (1 + 0.1 * torch.randn(K, device=DEV)).to(BF)
    lb = (0.1 * torch.randn(K, device=DEV)).to(BF)
    for branch in (False, True):
        del calls[:]
        res = torch.randn(1, 1, K, device=DEV) * 3 + 0.5
        br = torch.randn(1, 1, K, device=DEV).to(BF) if branch else None
        pos = torch.tensor([41], device=DEV, dtype=torch.int64) if branch and N == 768 else None
        s, y = ops.decode_linear_ln(res, br, lw, lb, qw, b, gelu=gelu, out_f32=f32, pos_inc=pos)
        _only_q8(calls, "nsa_gemv_ln_q8")
        assert len(calls) == 1
        if pos is not None:
            assert int(pos.item()) == 42
        s_ref = res + br.float() if branch else res
        assert torch.allclose(s, s_ref) and (branch or s is res)
        h = F.layer_norm(s_ref.view(1, K), (K,), lw.float(), lb.float(), 1e-5).to(BF).float()
        assert y.shape == (1, 1, N) and y.dtype == (torch.float32 if f32 else BF)
        err = _relerr(y, _ref(h, dq, b, gelu))
        assert err < 1e-2, (branch, err)


@pytest.mark.parametrize("rows", [2, 3, 5, 8])
@pytest.mark.parametrize("N,K,bias,gelu,f32", [(768, 768, True, False, False), (100, 64, True, True, False),
                                              (4800, 1600, True, False, True)])
def test_q8_gemv_multi_row(kernels, monkeypatch, rows, N, K, bias, gelu, f32):
    """nsa_gemv_q8 with the row cap raised (NSA_GEMV_MAX_ROWS): the K-loop kernel at 2..8 rows."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.ops import functional

    monkeypatch.setattr(functional, "GEMV_MAX_ROWS", 8)
    calls = _record(monkeypatch)
    qw, dq, b = _weights(N, K, bias, rows * 7 + N)
    x = torch.randn(rows, 1, K, device=DEV).to(BF)
    y = ops.decode_linear(x, qw, b, gelu=gelu, out_f32=f32)
    _only_q8(calls, "nsa_gemv_q8")
    assert y.shape == (rows, 1, N) and y.dtype == (torch.float32 if f32 else BF)
    err = _relerr(y, _ref(x.float().view(rows, K), dq, b, gelu))
    assert err < 1e-2, err


def test_q8_gemv_wide_row(kernels, monkeypatch):
    """One row wider than the no-loop kernels cover (K > 8192): the K-loop kernel, exact integers."""
    from nanosandbox_amd import ops

    calls = _record(monkeypatch)
    torch.manual_seed(3)
    N, K = 37, 8208
    x = torch.randint(-4, 5, (1, 1, K), device=DEV).to(BF)
    q = torch.randint(-127, 128, (N, K), device=DEV, dtype=torch.int32).to(torch.int8)
    scale = torch.pow(2.0, (torch.arange(N, device=DEV) % 6 - 3).float())
    ref = (x.double().view(1, K) @ q.double().t()) * scale.double()
    y = ops.decode_linear(x, ops.QuantWeight(q, scale), None, out_f32=True)
    _only_q8(calls, "nsa_gemv_q8")
    assert torch.equal(y.view(1, N), ref.float())


@pytest.mark.parametrize("C", [768, 2560])  # the vector prologue, and the scalar loop of K > 2048
def test_q8_embed_linear_ln_kernel(kernels, monkeypatch, C):
    from nanosandbox_amd import ops

    calls = _record(monkeypatch)
    V, T, N = 512, 128, 2304
    qw, dq, b = _weights(N, C, True, 1)
    wte = (torch.randn(V, C, device=DEV) * 0.5).to(BF)
    wpe = (torch.randn(T, C, device=DEV) * 0.5).to(BF)
    lw = (1 + 0.1 * torch.randn(C, device=DEV)).to(BF)
    lb = (0.1 * torch.randn(C, device=DEV)).to(BF)
    tok = torch.tensor([[311]], device=DEV)
    pos = torch.tensor([77], device=DEV)
    x, y = ops.decode_embed_linear_ln(tok, pos, wte, wpe, lw, lb, qw, b)
    _only_q8(calls, "nsa_gemv_emb_ln_q8")
    x_ref = wte[311].float() + wpe[77].float()
    assert x.dtype == torch.float32 and torch.equal(x.view(C), x_ref)
    h = F.layer_norm(x_ref.view(1, C), (C,), lw.float(), lb.float(), 1e-5).to(BF).float()
    err = _relerr(y, _ref(h, dq, b, False))
    assert y.shape == (1, 1, N) and err < 1e-2, err


# H = 12 (C = 768), and 40 (C = 2560): the second pass of the combine (K > 2048)
@pytest.mark.parametrize("pos,H", [pytest.param(p, h, id=str(p) if h == 12 else "%d-H%d" % (p, h))
                                   for h in (12, 40) for p in (0, 300, 1023)])
def test_q8_attention_partials_into_linear(kernels, monkeypatch, pos, H):
    """decode_attention(combine=False) -> decode_linear(QuantWeight): the combine in the
    nsa_gemv_attn_q8 prologue, against the combine kernel's bf16 output through the reference."""
    from nanosandbox_amd import ops

    torch.manual_seed(pos)
    D, T = 64, 1024
    C = H * D
    kc = torch.randn(1, H, T, D, device=DEV).to(BF)
    vc = torch.randn(1, H, T, D, device=DEV).to(BF)
    qkv = torch.randn(1, 1, 3 * C, device=DEV).to(BF)
    p = torch.tensor([pos], device=DEV, dtype=torch.int64)
    qw, dq, b = _weights(C, C, True, pos + 5)
    att = ops.decode_attention(qkv, kc.clone(), vc.clone(), p, H, append=True)  # [1, 1, C] bf16
    part = ops.decode_attention(qkv, kc, vc, p, H, append=True, combine=False)
    assert isinstance(part, ops.AttnPartials)
    calls = _record(monkeypatch)
    y = ops.decode_linear(part, qw, b)
    _only_q8(calls, "nsa_gemv_attn_q8")
    err = _relerr(y, _ref(att.float().view(1, C), dq, b, False))
    assert y.shape == (1, 1, C) and err < 1e-2, err


@pytest.mark.parametrize("rows", [2, 3, 8, 15, 16])
@pytest.mark.parametrize("N,K,bias,gelu,f32", [(768, 768, True, False, False), (3072, 768, True, True, False),
                                              (768, 3072, False, False, False), (50304, 768, False, False, True),
                                              (6400, 1600, True, True, False),
                                              (16, 64, True, False, False),    # one unit
                                              (48, 448, False, True, False),   # 7 units: not a multiple of the waves
                                              (100, 64, True, False, False)])  # N not a multiple of 16
def test_q8_skinny_gemm(kernels, monkeypatch, rows, N, K, bias, gelu, f32):
    from nanosandbox_amd import ops

    calls = _record(monkeypatch)
    qw, dq, b = _weights(N, K, bias, rows * 13 + N + K)
    x = torch.randn(rows, 1, K, device=DEV).to(BF)
    y = ops.decode_linear(x, qw, b, gelu=gelu, out_f32=f32)
    _only_q8(calls, "nsa_skinny_gemm_q8")
    assert y.shape == (rows, 1, N) and y.dtype == (torch.float32 if f32 else BF)
    err = _relerr(y, _ref(x.float().view(rows, K), dq, b, gelu))
    assert err < 1e-2, err


@pytest.mark.parametrize("rows", [2, 5, 8])
@pytest.mark.parametrize("branch", [False, True])
@pytest.mark.parametrize("N,K,bias,gelu,f32", [(2304, 768, True, False, False), (50304, 768, False, False, True),
                                              (6400, 1600, True, True, False), (48, 1920, False, False, False)])
def test_q8_skinny_ln_kernel(kernels, monkeypatch, rows, branch, N, K, bias, gelu, f32):
    from nanosandbox_amd import ops

    calls = _record(monkeypatch)
    qw, dq, b = _weights(N, K, bias, N + K + rows)
    res = torch.randn(rows, 1, K, device=DEV) * 3 + 0.5
    br = torch.randn(rows, 1, K, device=DEV).to(BF) if branch else None
    lw = (1 + 0.1 * torch.randn(K, device=DEV)).to(BF)
    lb = (0.1 * torch.randn(K, device=DEV)).to(BF)
    s, y = ops.decode_linear_ln(res, br, lw, lb, qw, b, gelu=gelu, out_f32=f32)
    _only_q8(calls, "nsa_skinny_ln_gemm_q8")
    s_ref = res + br.float() if branch else res
    assert torch.allclose(s, s_ref) and (branch or s is res)
    h = F.layer_norm(s_ref.view(rows, K), (K,), lw.float(), lb.float(), 1e-5).to(BF).float()
    assert y.shape == (rows, 1, N) and y.dtype == (torch.float32 if f32 else BF)
    err = _relerr(y, _ref(h, dq, b, gelu))
    assert err < 1e-2, err


@pytest.mark.parametrize("rows", [1, 2, 16])
@pytest.mark.parametrize("N,K", [(100, 64), (768, 1600), (50257, 768)])
@pytest.mark.parametrize("bias", [True, False])
def test_q8_exact_integer_pin(kernels, monkeypatch, rows, N, K, bias):
    """Indexing, sign handling and the k permutation, with nothing to round: small integer
    activations, any int8 weight (+-127 in every row), power-of-two scales that vary by row
    and a bias in eighths.  Every partial sum is an integer below 2^24 (at most
    K * 127 * 4), so fp32 accumulation is exact in any order and the fp32 output must equal
    the float64 reference bit for bit (rows = 1: nsa_gemv_q8; 2, 16: nsa_skinny_gemm_q8)."""
    from nanosandbox_amd import ops

    calls = _record(monkeypatch)
    torch.manual_seed(N + K + rows)
    x = torch.randint(-4, 5, (rows, 1, K), device=DEV).to(BF)
    q = torch.randint(-127, 128, (N, K), device=DEV, dtype=torch.int32).to(torch.int8)
    q[:, 0] = 127
    q[:, K - 1] = -127
    scale = torch.pow(2.0, (torch.arange(N, device=DEV) % 6 - 3).float())  # 2^-3 .. 2^2
    b = (torch.randint(-16, 17, (N,), device=DEV).float() / 8).to(BF) if bias else None
    qw = ops.QuantWeight(q, scale)
    ref = (x.double().view(rows, K) @ q.double().t()) * scale.double()
    if b is not None:
        ref = ref + b.double()
    assert torch.equal(ref.float().double(), ref)  # the premise: the result itself is an fp32 number
    y32 = ops.decode_linear(x, qw, b, out_f32=True)
    y16 = ops.decode_linear(x, qw, b)
    _only_q8(calls, "nsa_gemv_q8" if rows == 1 else "nsa_skinny_gemm_q8")
    assert y32.dtype == torch.float32 and torch.equal(y32.view(rows, N), ref.float())
    assert y16.dtype == BF and torch.equal(y16.view(rows, N), ref.to(BF))


def _model():  # tests/test_decode_gpu.py's
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


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


@pytest.mark.parametrize("B", [1, 4, 12])
def test_q8_graph_decode_matches_dequantized_model(kernels, monkeypatch, B):
    """B = 1: the fused single-row kernels; 4: the skinny kernels with the LayerNorm prologue;
    12: add+LayerNorm + the plain skinny kernel.  The int8 graph step equals the int8 eager
    step bit for bit and follows the model with the dequantized weights (the existing
    test's bounds: the extra bf16 rounding of those weights is 2^-9 per weight)."""
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    m2 = _dequantized_copy(m)
    T0, T = 40, 72
    idx = torch.randint(0, 512, (B, T), device=DEV)
    with torch.no_grad():
        full = m2.forward_logits(idx)
    dg = Decoder(m, B, use_graph=True, quantize="int8")
    de = Decoder(m, B, use_graph=False, quantize="int8")
    try:
        with torch.no_grad():
            lg, le = dg.prefill(idx[:, :T0]), de.prefill(idx[:, :T0])
            ref = full[:, T0 - 1]
            assert ((lg - ref).norm() / ref.norm()).item() < 2e-2
            for t in range(T0, T):
                lg = dg.step(idx[:, t]).clone()
                le = de.step(idx[:, t])
                assert torch.equal(lg, le), t
                err = ((lg - full[:, t]).norm() / full[:, t].norm()).item()
                assert err < 3e-2, (t, err)
        assert dg.replays == T - T0 and dg.position == T
        if B == 1:
            # one more eager step: every weight stream is int8, in as many launches as bf16
            calls = _record(monkeypatch)
            with torch.no_grad():
                de.step(idx[:, 0])
                nq = list(calls)
                assert not [c for c in nq if c in BF16_STREAM or c.startswith("nsa_gemm")], nq
                assert len([c for c in nq if c in Q8_STREAM]) == 4 * 3 + 1
                d0 = Decoder(m2, 1, use_graph=False)
                d0.prefill(idx[:, :T0])
                del calls[:]
                d0.step(idx[:, T0])
                assert len(calls) == len(nq), (calls, nq)
                d0.release()
    finally:
        de.release()
        dg.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_q8_decoder_refuses_large_batches(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    with pytest.raises(ValueError):
        Decoder(m, 17, quantize="int8")
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_q8_front_ends_on_gpu(kernels):
    m = _model()
    idx = torch.randint(0, 512, (2, 8), device=DEV)
    a = m.generate_cached(idx, 40, top_k=1, quantize="int8", use_graph=True)
    b = m.generate_cached(idx, 40, top_k=1, quantize="int8", use_graph=False)
    assert a.shape == (2, 48) and torch.equal(a, b) and torch.equal(a[:, :8], idx)

    prompts = [torch.randint(0, 512, (n,), device=DEV) for n in (3, 5, 9)]
    free = m.generate_batch(prompts, 24, top_k=1, quantize="int8", use_graph=False)
    stop = int(free[0][3 + 6])  # row 0 draws it as its 7th new token at the latest
    ya = m.generate_batch(prompts, 24, top_k=1, stop_token=stop, quantize="int8", use_graph=True)
    yb = m.generate_batch(prompts, 24, top_k=1, stop_token=stop, quantize="int8", use_graph=False)
    for p, u, v in zip(prompts, ya, yb):
        assert torch.equal(u, v) and torch.equal(u[:p.numel()], p)
        new = u[p.numel():]
        assert 1 <= new.numel() <= 24 and int(new.min()) >= 0 and int(new.max()) < 512
        assert new.numel() == 24 or int(new[-1]) == stop
        assert stop not in new[:-1].tolist()
    assert int(ya[0][-1]) == stop and ya[0].numel() <= 3 + 7
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
