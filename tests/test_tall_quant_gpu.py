"""``nsa_tall_gemm_q8`` / ``nsa_tall_gemm_mx4`` (csrc/kernels/decode_tall_q.hip), the decode linear of 65 .. 128 rows on
int8 and MXFP4 weights, and the decoder above 64 rows under ``NSA_QUANT_MAX_ROWS``.  Checked the way
``test_wide_quant_gpu.py`` checks the wide forms: NaN-filled guarded outputs, every launch made twice on one workspace
(a counter left above zero, or a stale partial read again, is a wrong or NaN element of the second)."""

import pytest
import torch

from test_decode_linear_gpu import DEV, Guarded, _exact
from test_decode_linear_refs import BF, F32, _sums_below_2_24, int_bias, int_x, linear_ref, plain_bound, rand_linear
from test_layernorm_gpu import _call
from test_mx4_gpu import _dequantized_copy as _mx4_copy, _rand_weight
from test_quant_gpu import BF16_STREAM, _dequantized_copy as _q8_copy, _model, _record
from test_wide_quant_gpu import GRANULE, _exact_weight

pytestmark = pytest.mark.gpu
_WS = {}


def _tall(fmt, x, q, scale, bias, y, rows, N, K, act=0, f32=0, ksplit=0):
    """One raw launch on the module's one zero-allocated workspace."""
    from nanosandbox_amd.ops import _lib
    need = _lib.call_ret(f"nsa_tall_gemm_{fmt}_ws_bytes", rows, N, K, ksplit)
    if "ws" not in _WS or _WS["ws"].numel() < need:
        _WS["ws"] = torch.zeros(max(need, 8 << 20), device=DEV, dtype=torch.uint8)
    _call(f"nsa_tall_gemm_{fmt}", x, q, scale, bias, y, rows, N, K, act, f32, ksplit, _WS["ws"], _WS["ws"].numel())


@pytest.mark.parametrize("fmt,K", [("mx4", 32), ("mx4", 96), ("mx4", "chunk + block"), ("mx4", 1600),
                                   ("q8", 64), ("q8", 192), ("q8", "chunk + granule"), ("q8", 1600)])
def test_tall_quant_exact(kernels, fmt, K):
    """The operands of ``test_wide_quant_exact``, whose every partial sum is exact in fp32 at 128 rows too, so any
    summation order and any split gives the float64 result bit for bit: bf16 and fp32, bias or none, rows at both RB
    values and their last-row edges, N with dead waves / a clamped weight row / a partial second tile, K split {1, 2,
    3, one granule each}, twice in a row.  K = 1600 in mx4 is 50 blocks: the last unit half dead."""
    from nanosandbox_amd.ops import functional
    if isinstance(K, str):
        K = functional.TALL_Q_CHUNK[fmt] + GRANULE[fmt]
    launches = 0
    for N in (1, 32, 130):
        q, scale, dq = _exact_weight(fmt, N, K)
        if fmt == "q8":
            assert _sums_below_2_24(int_x(128, K), q.cpu())
        b = int_bias(N).to(DEV)
        for rows in (65, 96, 97, 128):
            x = int_x(rows, K).to(DEV)
            for bias in (None, b):
                ref = linear_ref(x, dq, None, bias)[0]
                for f32 in (0, 1):
                    for ks in sorted({k for k in (1, 2, 3, K // GRANULE[fmt]) if k <= K // GRANULE[fmt]}):
                        for launch in (1, 2):
                            g = Guarded((rows, N), F32 if f32 else BF)
                            _tall(fmt, x, q, scale, bias, g.view, rows, N, K, 0, f32, ks)
                            _exact(g, ref, f32, (fmt, rows, N, K, bias is not None, f32, ks, launch))
                            launches += 1
    print(f"nsa_tall_gemm_{fmt} K = {K}: {launches} launches pinned")


@pytest.mark.parametrize("fmt", ["mx4", "q8"])
@pytest.mark.parametrize("rows,N,K", [(72, 80, 1600), (128, 784, 3072)])
def test_tall_quant_random_per_element(kernels, fmt, rows, N, K):
    """Plain / fp32 / GELU per element within ``plain_bound`` under the rule's own split, against the references of
    ``test_wide_quant_random_per_element``: mx4 ``linear_ref`` on ``ops.dequantize(w)``, int8 ``linear_ref(x, q,
    scale, b)`` (the scale multiplies the finished sum, as the kernel does after its cross-split reduction); the two
    launches give the same bits.  Worst error / bound on an MI355X: mx4 0.9081 and 0.9451, int8 0.9016 and 0.9437 for
    the two shapes."""
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
            _tall(fmt, x, q, scale, b, y.view, rows, N, K, act, f32)
            torch.cuda.synchronize()
            assert y.written(), (act, f32)
            ys.append(y.view)
        assert torch.equal(ys[0], ys[1]), (act, f32)
        ratio = float(((ys[0].double() - ref).abs() / plain_bound(ref, mag, u, act, f32)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{(fmt, rows, N, K, act, f32)}: error / bound {ratio:.4f}"
    print(f"nsa_tall_gemm_{fmt} {(rows, N, K)}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("quantize,fmt", [("int8", "q8"), ("mxfp4", "mx4")])
@pytest.mark.parametrize("B", [65, 100])
def test_tall_quant_decoder(kernels, monkeypatch, quantize, fmt, B):
    """The quantized decoder refuses 65 and 100 rows at the default and at ``NSA_QUANT_MAX_ROWS`` = 64, builds at 128
    and still refuses 129.  Captured-graph and eager logits are the same bits and the graph replays; against the bf16
    decoder on a deep copy holding the dequantized weights the logits stay within 3e-2 relative at every step (the
    existing quantized decoder tests' figure); one recorded eager step streams its 4 linears per layer and the
    lm_head through the quantized tall kernel alone, in as many launches as the bf16 step."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder
    m = _model()
    for cap in (None, 64):
        if cap:
            monkeypatch.setattr(ops.functional, "QUANT_MAX_ROWS", cap)
        with pytest.raises(ValueError):
            Decoder(m, B, quantize=quantize)
    monkeypatch.setattr(ops.functional, "QUANT_MAX_ROWS", 128)
    with pytest.raises(ValueError):
        Decoder(m, 129, quantize=quantize)
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
        assert not [c for c in nq if c in BF16_STREAM or c == "nsa_tall_gemm" or c.startswith("nsa_gemm")], nq
        assert nq.count("nsa_tall_gemm_" + fmt) == 4 * 3 + 1 and len(nq) == len(calls), (nq, calls)
        assert calls.count("nsa_tall_gemm") == 4 * 3 + 1, calls
    finally:
        for d in (d0, de, dg):  # the reverse of their creation: each puts back the shadows it found
            d.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
