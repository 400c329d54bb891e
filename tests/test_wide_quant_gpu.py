"""``nsa_wide_gemm_q8`` / ``nsa_wide_gemm_mx4`` (csrc/kernels/decode_wide_q.hip), the decode linear of 17 .. 64 rows on
int8 and MXFP4 weights, and the decoder above 16 rows under ``NSA_QUANT_MAX_ROWS``.  Checked the way
``test_decode_wide_gpu.py`` checks the bf16 kernel: NaN-filled guarded outputs, every launch made twice on one
workspace (a counter left above zero, or a stale partial read again, is a wrong or NaN element of the second)."""

import pytest
import torch

from test_decode_linear_gpu import DEV, Guarded, _exact
from test_decode_linear_refs import (BF, F32, _sums_below_2_24, int_bias, int_weight, int_x, linear_ref, plain_bound,
                                     rand_linear)
from test_layernorm_gpu import _call
from test_mx4_gpu import _dequantized_copy as _mx4_copy, _rand_weight
from test_quant_gpu import BF16_STREAM, _dequantized_copy as _q8_copy, _model, _record

pytestmark = pytest.mark.gpu
GRANULE = {"q8": 64, "mx4": 32}  # k per split granule: what K is a multiple of, and the finest split
_WS = {}


def _wide(fmt, x, q, scale, bias, y, rows, N, K, act=0, f32=0, ksplit=0):
    """One raw launch on the module's one zero-allocated workspace."""
    from nanosandbox_amd.ops import _lib
    need = _lib.call_ret(f"nsa_wide_gemm_{fmt}_ws_bytes", rows, N, K, ksplit)
    if "ws" not in _WS or _WS["ws"].numel() < need:
        _WS["ws"] = torch.zeros(max(need, 1 << 20), device=DEV, dtype=torch.uint8)
    _call(f"nsa_wide_gemm_{fmt}", x, q, scale, bias, y, rows, N, K, act, f32, ksplit, _WS["ws"], _WS["ws"].numel())


def _exact_weight(fmt, N, K):
    """-> (q, scale, the float64 weight): int8 with +-127 at both row ends and power-of-two row scales; or random
    nibbles with scale bytes 124 .. 127 drawn per block (``test_mx4_exact_pin``'s operands)."""
    from nanosandbox_amd import ops
    if fmt == "q8":
        q, scale = (t.to(DEV) for t in int_weight(N, K, True))
        assert _sums_below_2_24(int_x(64, K), q.cpu())
        return q, scale, q.double() * scale.double()[:, None]
    g = torch.Generator().manual_seed(N + K)
    w = ops.MxWeight(torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8).to(DEV),
                     torch.randint(124, 128, (N, K // 32), generator=g, dtype=torch.uint8).to(DEV))
    return w.q, w.scale, ops.dequantize(w).double()


@pytest.mark.parametrize("fmt,K", [("mx4", 32), ("mx4", 160), ("mx4", "chunk + block"), ("mx4", 1600),
                                   ("q8", 64), ("q8", 320), ("q8", "chunk + unit"), ("q8", 1600)])
def test_wide_quant_exact(kernels, fmt, K):
    """Operands whose every partial sum is exact in fp32 (mx4: products are multiples of 2^-4 with |sum| <= 24 K 2^4;
    int8: integers up to 508 K, scaled by a power of two after the sum), so any summation order and any split gives
    the float64 result bit for bit: bf16 and fp32, bias or none, rows at both MT values and their last-row edges, N
    with a dead wave / a clamped weight row / a partial tile, K split {1, 2, 3, one granule each}, twice in a row."""
    from nanosandbox_amd.ops import functional
    if isinstance(K, str):
        K = functional.WIDE_Q_CHUNK[fmt] + GRANULE[fmt]
    launches = 0
    for N in (1, 16, 100):
        q, scale, dq = _exact_weight(fmt, N, K)
        b = int_bias(N).to(DEV)
        for rows in (17, 32, 33, 64):
            x = int_x(rows, K).to(DEV)
            for bias in (None, b):
                ref = linear_ref(x, dq, None, bias)[0]
                for f32 in (0, 1):
                    for ks in sorted({k for k in (1, 2, 3, K // GRANULE[fmt]) if k <= K // GRANULE[fmt]}):
                        for launch in (1, 2):
                            g = Guarded((rows, N), F32 if f32 else BF)
                            _wide(fmt, x, q, scale, bias, g.view, rows, N, K, 0, f32, ks)
                            _exact(g, ref, f32, (fmt, rows, N, K, bias is not None, f32, ks, launch))
                            launches += 1
    print(f"nsa_wide_gemm_{fmt} K = {K}: {launches} launches pinned")


@pytest.mark.parametrize("fmt", ["mx4", "q8"])
@pytest.mark.parametrize("rows,N,K", [(24, 80, 1600), (64, 784, 3072)])
def test_wide_quant_random_per_element(kernels, fmt, rows, N, K):
    """Plain / fp32 / GELU per element within ``plain_bound`` under the rule's own split (1 and 3 for the two shapes).
    mx4: against ``linear_ref`` on ``ops.dequantize(w)`` (operands exact, fp32 accumulation).  int8: against
    ``linear_ref(x, q, scale, b)``, the reference of the existing int8 pins: the weights are exact integers and
    the scale multiplies the finished sum, which is what the kernel does after its cross-split reduction.
    Worst error / bound on an MI355X: mx4 0.9267 and 0.9487, int8 0.9100 and 0.9487 for the two shapes."""
    from nanosandbox_amd import ops
    if fmt == "q8":
        x, q, scale, b = (t.to(DEV) for t in rand_linear(rows, N, K, True))
        W, rs = q, scale
    else:
        w = _rand_weight(N, K, rows + N + K)
        g = torch.Generator().manual_seed(K)
        x, b = torch.randn(rows, K, generator=g).to(BF).to(DEV), (torch.randn(N, generator=g) * 0.1).to(BF).to(DEV)
        q, scale, W, rs = w.q, w.scale, ops.dequantize(w), None
    worst = 0.0
    for act, f32 in ((0, 0), (0, 1), (1, 0)):
        ref, mag, u = linear_ref(x, W, rs, b, act)
        ys = []
        for _ in range(2):
            y = Guarded((rows, N), F32 if f32 else BF)
            _wide(fmt, x, q, scale, b, y.view, rows, N, K, act, f32)
            torch.cuda.synchronize()
            assert y.written(), (act, f32)
            ys.append(y.view)
        assert torch.equal(ys[0], ys[1]), (act, f32)
        ratio = float(((ys[0].double() - ref).abs() / plain_bound(ref, mag, u, act, f32)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{(fmt, rows, N, K, act, f32)}: error / bound {ratio:.4f}"
    print(f"nsa_wide_gemm_{fmt} {(rows, N, K)}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("quantize,fmt", [("int8", "q8"), ("mxfp4", "mx4")])
@pytest.mark.parametrize("B", [17, 40])
def test_wide_quant_decoder(kernels, monkeypatch, quantize, fmt, B):
    """``NSA_QUANT_MAX_ROWS`` = 64: the quantized decoder accepts 17 and 40 rows.  Captured-graph and eager logits are
    the same bits and the graph replays; against the bf16 decoder on a deep copy holding the dequantized weights the
    logits stay within 3e-2 relative at every step (the existing quantized decoder tests' figure); one recorded
    eager step streams its 4 linears per layer and the lm_head through the quantized wide kernel alone, in as
    many launches as the bf16 step."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder
    m = _model()
    with pytest.raises(ValueError):
        Decoder(m, B, quantize=quantize)
    monkeypatch.setattr(ops.functional, "QUANT_MAX_ROWS", 64)
    m2 = (_q8_copy if fmt == "q8" else _mx4_copy)(m)
    T0, T = 24, 32
    idx = torch.randint(0, 512, (B, T0), device=DEV)
    dg, de, d0 = (Decoder(m, B, use_graph=True, quantize=quantize), Decoder(m, B, use_graph=False, quantize=quantize),
                  Decoder(m2, B, use_graph=False))
    try:
        with torch.no_grad():
            lg, le, l0 = dg.prefill(idx), de.prefill(idx), d0.prefill(idx)
            for t in range(T0, T):
                err = ((lg - l0).norm() / l0.norm()).item()
                assert err < 3e-2, (t, err)
                tok = l0.argmax(-1)
                lg, le, l0 = dg.step(tok).clone(), de.step(tok), d0.step(tok)
                assert torch.equal(lg, le), t
            assert dg.replays > 0
            calls = _record(monkeypatch)
            de.step(tok)
            nq = list(calls)
            del calls[:]
            d0.step(tok)
        print(f"{quantize} B = {B}: {dg.replays} replays, {len(nq)} launches in the eager step, last error {err:.2e}")
        assert not [c for c in nq if c in BF16_STREAM or c == "nsa_wide_gemm" or c.startswith("nsa_gemm")], nq
        assert nq.count("nsa_wide_gemm_" + fmt) == 4 * 3 + 1 and len(nq) == len(calls), (nq, calls)
        assert calls.count("nsa_wide_gemm") == 4 * 3 + 1, calls
    finally:
        for d in (d0, de, dg):  # the reverse of their creation: each puts back the shadows it found
            d.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
