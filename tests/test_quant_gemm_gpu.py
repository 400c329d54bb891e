"""``nsa_quant_gemm_q8`` / ``nsa_quant_gemm_mx4`` (csrc/kernels/quant_gemm.hip), the GEMM of any number of rows on int8
and MXFP4 weights, and the decoder that runs its prompt passes on it (``quantize_prefill=True``).  Checked the way
``test_wide_quant_gpu.py`` checks the wide kernel: NaN-filled guarded outputs, every launch made twice."""

import pytest
import torch

from test_decode_linear_gpu import DEV, Guarded, _exact
from test_decode_linear_refs import BF, int_bias, int_x, linear_ref, plain_bound, rand_linear
from test_layernorm_gpu import _call
from test_mx4_gpu import _dequantized_copy as _mx4_copy, _rand_weight
from test_quant_gpu import _dequantized_copy as _q8_copy, _model, _record
from test_quant_refs import _quant_params
from test_wide_quant_gpu import GRANULE, _exact_weight

pytestmark = pytest.mark.gpu
FMT = {"int8": "q8", "mxfp4": "mx4"}


def _gemm(fmt, *args):
    _call(f"nsa_quant_gemm_{fmt}", *args)


@pytest.mark.parametrize("fmt,K", [("mx4", "granule"), ("mx4", "chunk + granule"), ("mx4", 1600),
                                   ("q8", "granule"), ("q8", "chunk + granule"), ("q8", 1600)])
def test_quant_gemm_exact(kernels, fmt, K):
    """Operands whose every fp32 partial sum is exact (``test_wide_quant_exact``'s), so the result is the float64 one
    bit for bit in any summation order: M at a row tile's last row and the first row of a second tile, N with a
    clamped weight row / a partial tile with dead waves / a second column tile, K of one granule, one LDS chunk
    plus a granule (a partial last chunk) and 1600, bias or none, twice in a row."""
    from nanosandbox_amd.ops import _lib, functional
    assert _lib.call_ret(f"nsa_quant_gemm_{fmt}_chunk") == functional.QUANT_GEMM_CHUNK[fmt]
    K = {"granule": GRANULE[fmt], "chunk + granule": functional.QUANT_GEMM_CHUNK[fmt] + GRANULE[fmt]}.get(K, K)
    for N in (1, 100, 129):
        q, scale, dq = _exact_weight(fmt, N, K)
        b = int_bias(N).to(DEV)
        for M in (1, 127, 128, 129):
            x = int_x(M, K).to(DEV)
            for bias in (None, b):
                ref = linear_ref(x, dq, None, bias)[0]
                for launch in (1, 2):
                    g = Guarded((M, N), BF)
                    _gemm(fmt, x, q, scale, bias, g.view, M, N, K, 0)
                    _exact(g, ref, 0, (fmt, M, N, K, bias is not None, launch))


@pytest.mark.parametrize("fmt", ["mx4", "q8"])
@pytest.mark.parametrize("M,N,K", [(130, 200, 1600), (257, 784, 3072)])
def test_quant_gemm_random_per_element(kernels, fmt, M, N, K):
    """Plain and GELU per element within ``plain_bound``; mx4 against ``linear_ref`` on ``ops.dequantize(w)``, int8
    against ``linear_ref(x, q, scale, b)`` (the scale multiplies the finished sum); two launches give equal bits.
    Worst error / bound on an MI355X: mx4 0.9393 and 0.9328, int8 0.9364 and 0.9470 for the two shapes."""
    from nanosandbox_amd import ops
    if fmt == "q8":
        x, q, scale, b = (t.to(DEV) for t in rand_linear(M, N, K, True))
        W, rs = q, scale
    else:
        w = _rand_weight(N, K, M + N + K)
        g = torch.Generator().manual_seed(K)
        x, b = torch.randn(M, K, generator=g).to(BF).to(DEV), (torch.randn(N, generator=g) * 0.1).to(BF).to(DEV)
        q, scale, W, rs = w.q, w.scale, ops.dequantize(w), None
    worst = 0.0
    for act in (0, 1):
        ref, mag, u = linear_ref(x, W, rs, b, act)
        ys = []
        for _ in range(2):
            y = Guarded((M, N), BF)
            _gemm(fmt, x, q, scale, b, y.view, M, N, K, act)
            torch.cuda.synchronize()
            assert y.written(), act
            ys.append(y.view)
        assert torch.equal(ys[0], ys[1]), act
        ratio = float(((ys[0].double() - ref).abs() / plain_bound(ref, mag, u, act, 0)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, f"{(fmt, M, N, K, act)}: error / bound {ratio:.4f}"
    print(f"nsa_quant_gemm_{fmt} {(M, N, K)}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("quantize", ["int8", "mxfp4"])
@pytest.mark.parametrize("B", [2, 20])
def test_quantize_prefill_decoder(kernels, monkeypatch, quantize, B):
    """No block linear has a ``compute`` shadow while the decoder lives and none is left after ``release()``; one
    prefill launches the quantized GEMM 4 x n_layer times and that many fewer ``nsa_gemm*`` than the flag-off
    decoder's; prefill logits within 3e-2 relative of the bf16 decoder on the dequantized copy (the quantized
    decoder tests' figure); the following steps are the same bits captured and eager, and the graph replays."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder
    fmt = FMT[quantize]
    monkeypatch.setattr(ops.functional, "QUANT_MAX_ROWS", 64)
    m = _model()
    m2 = (_q8_copy if fmt == "q8" else _mx4_copy)(m)
    T0, T = 24, 30
    idx = torch.randint(0, 512, (B, T0), device=DEV)
    mode = dict(quantize=quantize, quantize_prefill=True)
    dg, de, d0 = Decoder(m, B, use_graph=True, **mode), Decoder(m, B, use_graph=False, **mode), Decoder(m2, B, use_graph=False)
    calls = _record(monkeypatch)

    def gemms():
        n = (calls.count("nsa_quant_gemm_" + fmt), len([c for c in calls if c.startswith("nsa_gemm")]))
        del calls[:]
        return n
    try:
        assert not [p for p in _quant_params(m)[:-1] if hasattr(p, "compute")] and hasattr(m.lm_head.weight, "compute")
        with torch.no_grad():
            lg = dg.prefill(idx)
            del calls[:]
            le, on = de.prefill(idx), gemms()
            l0 = d0.prefill(idx)
            for t in range(T0, T):
                err = ((lg - l0).norm() / l0.norm()).item()
                assert err < 3e-2, (t, err)
                tok = l0.argmax(-1)
                lg, le, l0 = dg.step(tok).clone(), de.step(tok), d0.step(tok)
                assert torch.equal(lg, le), t
            assert dg.replays > 0
        assert not [p for p in _quant_params(m)[:-1] if hasattr(p, "compute")]
    finally:
        for d in (d0, de, dg):
            d.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
    df = Decoder(m, B, use_graph=False, quantize=quantize)
    try:
        del calls[:]
        with torch.no_grad():
            df.prefill(idx)
        off = gemms()
    finally:
        df.release()
    print(f"{quantize} B = {B}: prefill launches (quant gemm, nsa_gemm*) flag on {on}, off {off}; last error {err:.2e}")
    assert on[0] == 4 * 3 and off[0] == 0 and on[1] == off[1] - 4 * 3, (on, off)


@pytest.mark.parametrize("quantize", ["int8", "mxfp4"])
def test_quantize_prefill_queue_admits(kernels, quantize):
    """Three prompts through two rows, so an ``admit`` prefills on the quantized weights: the greedy tokens (compared
    as tokens, not logits) are those of the flag-off quantized decoder."""
    m = _model()
    prompts = [torch.randint(0, 512, (n,), device=DEV) for n in (3, 5, 9)]
    on = m.generate_batch(prompts, 8, top_k=1, quantize=quantize, quantize_prefill=True, batch_size=2)
    off = m.generate_batch(prompts, 8, top_k=1, quantize=quantize, batch_size=2)
    for p, a, b in zip(prompts, on, off):
        assert torch.equal(a, b), (p.numel(), a.tolist(), b.tolist())
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
