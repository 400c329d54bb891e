"""MXFP4 weight-only decode kernels (csrc/kernels/decode_mx4.hip) and ``Decoder(quantize="mxfp4")`` on gfx950.
Dequantized MXFP4 values are exact in bf16 and fp32, so the kernels differ from a float64 product on
``ops.dequantize(w)`` by fp32 summation order alone."""

import copy

import pytest
import torch
import torch.nn.functional as F

from test_decode_linear_gpu import DEV, Guarded, _exact
from test_decode_linear_refs import BF, F32, int_bias, int_x, linear_ref, plain_bound
from test_layernorm_gpu import _call
from test_quant_gpu import BF16_STREAM, _model, _record, _relerr

pytestmark = pytest.mark.gpu
MX4_STREAM = {n + "_mx4" for n in BF16_STREAM}


def _entry(rows):
    return "nsa_gemv_mx4" if rows == 1 else "nsa_skinny_gemm_mx4"


def _rand_weight(N, K, seed):
    from nanosandbox_amd import ops
    g = torch.Generator().manual_seed(seed)
    return ops.quantize_mxfp4((torch.randn(N, K, generator=g) * 0.05).to(DEV))


# one block, three, a unit + a block, 6 units in half-block pieces, 12.5 units in whole-block pieces
@pytest.mark.parametrize("K", [32, 96, 160, 768, 1600])
def test_mx4_exact_pin(kernels, K):
    """Random codes, scale bytes 124 .. 127 drawn per block, integer x in -4 .. 4: every product is a multiple of
    2^-4 and |sum| <= 24 K 2^4 < 2^24, so any summation order is exact and y is the float64 result bit for bit,
    bf16 and fp32, with and without a bias, into NaN-filled guarded buffers (rows 1: nsa_gemv_mx4; 2, 15, 16:
    nsa_skinny_gemm_mx4).  A wrong scale / block pairing, nibble order or tail lane group is a wrong integer."""
    from nanosandbox_amd import ops
    g = torch.Generator().manual_seed(K)
    for N in (1, 16, 100):
        w = ops.MxWeight(torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8).to(DEV),
                         torch.randint(124, 128, (N, K // 32), generator=g, dtype=torch.uint8).to(DEV))
        dq, b = ops.dequantize(w), int_bias(N).to(DEV)
        for rows in (1, 2, 15, 16):
            x = int_x(rows, K).to(DEV)
            for bias in (None, b):
                ref = linear_ref(x, dq, None, bias)[0]
                for f32 in (0, 1):
                    y = Guarded((rows, N), F32 if f32 else BF)
                    _call(_entry(rows), x, w.q, w.scale, bias, y.view, rows, N, K, 0, f32)
                    _exact(y, ref, f32, (rows, N, K, bias is not None, f32))


@pytest.mark.parametrize("rows,N,K", [(1, 100, 96), (16, 80, 1600), (8, 784, 3072)])
def test_mx4_random_per_element(kernels, rows, N, K):
    """Plain / fp32 / GELU per element within ``plain_bound`` (operands exact, fp32 accumulation: what the bound
    was derived for).  Worst error / bound on an MI355X: 0.8814, 0.9229, 0.9012 for the three shapes (a bf16
    output's own rounding is the 2^-8 |ref| term)."""
    from nanosandbox_amd import ops
    w = _rand_weight(N, K, rows + N + K)
    g = torch.Generator().manual_seed(K)
    x, b = torch.randn(rows, K, generator=g).to(BF).to(DEV), (torch.randn(N, generator=g) * 0.1).to(BF).to(DEV)
    worst = 0.0
    for act, f32 in ((0, 0), (0, 1), (1, 0)):
        ref, mag, u = linear_ref(x, ops.dequantize(w), None, b, act)
        y = Guarded((rows, N), F32 if f32 else BF)
        _call(_entry(rows), x, w.q, w.scale, b, y.view, rows, N, K, act, f32)
        torch.cuda.synchronize()
        assert y.written(), (act, f32)
        ratio = float(((y.view.double() - ref).abs() / plain_bound(ref, mag, u, act, f32)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{(rows, N, K, act, f32)}: error / bound {ratio:.4f}"
    print(f"mx4 {(rows, N, K)}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("rows", [1, 2, 5, 8])
@pytest.mark.parametrize("N,K,gelu", [(100, 768, True), (304, 1600, False)])
def test_mx4_prologue_forms(kernels, monkeypatch, rows, N, K, gelu):
    """nsa_gemv_ln_mx4 (one row) and nsa_skinny_ln_gemm_mx4 with and without a branch, and nsa_gemv_emb_ln_mx4,
    through ``ops``: fp32 torch on dequantize(w) with the LayerNorm output bf16-rounded, relative Frobenius
    error < 1e-2 (tests/test_quant_gpu.py's tolerance for the same comparison)."""
    from nanosandbox_amd import ops
    calls = _record(monkeypatch)
    w = _rand_weight(N, K, rows + N)
    dq = ops.dequantize(w)
    torch.manual_seed(rows)
    b = (torch.randn(N, device=DEV) * 0.1).to(BF)
    lw, lb = (1 + 0.1 * torch.randn(K, device=DEV)).to(BF), (0.1 * torch.randn(K, device=DEV)).to(BF)

    def ref(s):
        y = F.layer_norm(s.view(-1, K), (K,), lw.float(), lb.float(), 1e-5).to(BF).float() @ dq.t() + b.float()
        return F.gelu(y) if gelu else y

    for branch in (False, True):
        del calls[:]
        res = torch.randn(rows, 1, K, device=DEV) * 3 + 0.5
        br = torch.randn(rows, 1, K, device=DEV).to(BF) if branch else None
        s, y = ops.decode_linear_ln(res, br, lw, lb, w, b, gelu=gelu)
        assert calls == ["nsa_gemv_ln_mx4" if rows == 1 else "nsa_skinny_ln_gemm_mx4"], calls
        s_ref = res + br.float() if branch else res
        assert torch.allclose(s, s_ref) and (branch or s is res)
        assert y.shape == (rows, 1, N) and _relerr(y, ref(s_ref)) < 1e-2, (branch, _relerr(y, ref(s_ref)))
    if rows == 1 and not gelu:
        wte, wpe = (torch.randn(64, K, device=DEV) * 0.5).to(BF), (torch.randn(32, K, device=DEV) * 0.5).to(BF)
        del calls[:]
        x, y = ops.decode_embed_linear_ln(torch.tensor([[41]], device=DEV), torch.tensor([7], device=DEV), wte, wpe,
                                          lw, lb, w, b)
        assert calls == ["nsa_gemv_emb_ln_mx4"], calls
        assert torch.equal(x.view(K), wte[41].float() + wpe[7].float()) and _relerr(y, ref(x)) < 1e-2


def _dequantized_copy(m):
    from nanosandbox_amd import ops
    m2 = copy.deepcopy(m)
    ps = [m2.lm_head.weight]
    for blk in m2.transformer.h:
        ps += [blk.attn.c_attn.weight, blk.attn.c_proj.weight, blk.mlp.c_fc.weight, blk.mlp.c_proj.weight]
    with torch.no_grad():
        for p in ps:
            p.copy_(ops.dequantize(ops.quantize_mxfp4(p)))
    return m2


@pytest.mark.parametrize("B", [1, 2])
def test_mx4_decoder(kernels, monkeypatch, B):
    """Eager and captured-graph greedy tokens agree and the graph replays; against the plain bf16 decoder on a deep
    copy holding the dequantized weights: the same arg-max at every step and logits within 3e-2 relative
    (tests/test_quant_gpu.py's figure for its analogous check); one recorded eager step streams only ``_mx4``
    kernels (nsa_gemv_attn_mx4 among them at B = 1), in as many launches as the bf16 step."""
    from nanosandbox_amd.runtime.decode import Decoder
    m = _model()
    m2 = _dequantized_copy(m)
    T0, T = 40, 56
    idx = torch.randint(0, 512, (B, T0), device=DEV)
    dg, de, d0 = (Decoder(m, B, use_graph=True, quantize="mxfp4"), Decoder(m, B, use_graph=False, quantize="mxfp4"),
                  Decoder(m2, B, use_graph=False))
    try:
        with torch.no_grad():
            lg, le, l0 = dg.prefill(idx), de.prefill(idx), d0.prefill(idx)
            for t in range(T0, T):
                tok = l0.argmax(-1)
                assert torch.equal(lg.argmax(-1), tok) and torch.equal(le.argmax(-1), tok), t
                err = ((lg - l0).norm() / l0.norm()).item()
                assert err < 3e-2, (t, err)
                lg, le, l0 = dg.step(tok).clone(), de.step(tok), d0.step(tok)
            assert dg.replays > 0
            calls = _record(monkeypatch)
            de.step(tok)
            nq = list(calls)
            del calls[:]
            d0.step(tok)
        assert not [c for c in nq if c in BF16_STREAM or c.startswith("nsa_gemm")], nq
        assert len([c for c in nq if c in MX4_STREAM]) == 4 * 3 + 1 and len(nq) == len(calls), (nq, calls)
        assert B > 1 or "nsa_gemv_attn_mx4" in nq
    finally:
        for d in (d0, de, dg):  # the reverse of their creation: each puts back the shadows it found
            d.release()
    with pytest.raises(ValueError):
        Decoder(m, 17, quantize="mxfp4")
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
