"""``nsa_tall_gemm`` (csrc/kernels/decode_tall.hip), the decode linear of 65 .. 256 rows, checked the way
``test_decode_wide_gpu.py`` checks the wide kernel: guarded NaN-filled outputs, two launches on one workspace."""

import pytest
import torch

from test_decode_linear_gpu import DEV, Guarded, _exact
from test_decode_linear_refs import (BF, F32, _sums_below_2_24, int_bias, int_weight, int_x, linear_ref, plain_bound,
                                     rand_linear)
from test_layernorm_gpu import HIP_INVALID_VALUE, _call

pytestmark = pytest.mark.gpu
ROWS = [65, 96, 97, 128, 129, 192, 193, 256]  # both sides of each row-block edge (3 / 4 / 6 / 8 blocks of 32)
NS = [16, 144, 784]                  # half a wave's columns, a tile + a 16-column tail, many tiles + a tail
_WS = {}


def _ws(rows, N, K, ksplit):
    from nanosandbox_amd.ops import _lib
    need = _lib.call_ret("nsa_tall_gemm_ws_bytes", rows, N, K, ksplit)
    if "ws" not in _WS or _WS["ws"].numel() < need:
        _WS["ws"] = torch.zeros(max(need, 64 << 20), device=DEV, dtype=torch.uint8)
    return _WS["ws"], need


def _tall(x, W, bias, y, rows, N, K, act=0, f32=0, ksplit=0, ws="own", ws_bytes=None):
    buf, _ = _ws(rows, N, K, ksplit)
    _call("nsa_tall_gemm", x, W, bias, y, rows, N, K, act, f32, ksplit, buf if ws == "own" else ws,
          buf.numel() if ws_bytes is None else ws_bytes)


@pytest.mark.parametrize("K", ["unit", "3 units", "chunk + unit", 1056])
def test_tall_gemm_exact(kernels, K):
    """Integer operands (sum |x| |W| <= 32 K < 2^24: any order of partial sums is exact), bias or none, bf16
    and fp32, K split by {rule, 1, 2, 3, one unit each}: bit for bit on both of two launches in a row."""
    from nanosandbox_amd.ops import functional
    K = {"unit": 32, "3 units": 96, "chunk + unit": functional.TALL_CHUNK + 32}.get(K, K)
    assert _sums_below_2_24(int_x(256, 1056), int_weight(784, 1056, False)[0])
    for N in NS:
        W, b = int_weight(N, K, False)[0].to(DEV), int_bias(N).to(DEV)
        for rows in ROWS:
            x = int_x(rows, K).to(DEV)
            for bias in (None, b):
                ref = linear_ref(x, W, None, bias)[0]
                for f32 in (0, 1):
                    for ks in sorted({k for k in (0, 1, 2, 3, K // 32) if k <= K // 32}):
                        for launch in (1, 2):
                            g = Guarded((rows, N), F32 if f32 else BF)
                            _tall(x, W, bias, g.view, rows, N, K, 0, f32, ks)
                            _exact(g, ref, f32, (rows, N, K, bias is not None, f32, ks, launch))


@pytest.mark.parametrize("rows,N,K", [(65, 16, 32), (129, 144, 1056), (256, 784, 1600)])
def test_tall_gemm_random_per_element(kernels, rows, N, K):
    """Plain / fp32 / GELU per element within ``plain_bound`` (the skinny kernel's bound) for the rule's split,
    no split and one unit per workgroup; a second launch gives the first one's bits.  Worst error / bound on
    an MI355X: 0.9644, 0.9339, 0.9460 for the three shapes (a bf16 output's own rounding is the 2^-8 |ref| term)."""
    x, W, _, b = (t if t is None else t.to(DEV) for t in rand_linear(rows, N, K, False))
    worst = 0.0
    for act, f32 in ((0, 0), (0, 1), (1, 0)):
        ref, mag, u = linear_ref(x, W, None, b, act)
        bound = plain_bound(ref, mag, u, act, f32)
        for ks in (0, 1, K // 32):
            ys = []
            for _ in range(2):
                g = Guarded((rows, N), F32 if f32 else BF)
                _tall(x, W, b, g.view, rows, N, K, act, f32, ks)
                torch.cuda.synchronize()
                assert g.written(), (act, f32, ks)
                ys.append(g.view)
            assert torch.equal(ys[0], ys[1]), (act, f32, ks)
            ratio = float(((ys[0].double() - ref).abs() / bound).max())
            worst = max(worst, ratio)
            assert ratio <= 1.0, f"{(rows, N, K, act, f32, ks)}: error / bound {ratio:.4f}"
    print(f"nsa_tall_gemm {(rows, N, K)}: worst error / bound {worst:.4f}")


@pytest.mark.parametrize("bad", [dict(rows=0), dict(rows=257), dict(N=24), dict(K=48), dict(act=1, f32=1),
                                 dict(ksplit=3), dict(ksplit=2, ws=None), dict(ksplit=2, ws_bytes="short")],
                         ids=lambda d: "-".join(f"{k}{v}" for k, v in d.items()))
def test_tall_gemm_refusals(kernels, bad):
    """hipErrorInvalidValue and y untouched; put right, the call launches.  K = 64: ksplit 3 is one too many."""
    x, W = torch.zeros(257, 64, device=DEV, dtype=BF), torch.zeros(32, 64, device=DEV, dtype=BF)
    y = Guarded((257, 32), F32)
    kw = dict(rows=70, N=16, K=64, act=0, f32=0, ksplit=0)
    need = _ws(70, 16, 64, 2)[1]
    assert need > 0 and _ws(70, 16, 64, 1)[1] == 0
    args = {**kw, **bad, **({"ws_bytes": need - 1} if bad.get("ws_bytes") == "short" else {})}
    with pytest.raises(RuntimeError, match=f"hipError {HIP_INVALID_VALUE}$"):
        _tall(x, W, None, y.view, **args)
    torch.cuda.synchronize()
    assert y.untouched()
    _tall(x, W, None, y.view, **dict(kw, ksplit=2, ws_bytes=need))
    torch.cuda.synchronize()
    assert not y.untouched()


def test_ops_route_65_to_256_rows_to_the_tall_kernel(kernels, monkeypatch):
    """``ops.decode_linear``, caps 16 / 64 / 256: one ``nsa_tall_gemm`` call and the exact integers at 65 and 256
    rows; 64 rows, 257 rows, a ``QuantWeight``, an ``MxWeight`` and 65 rows under a tall cap of 64 never reach it."""
    from nanosandbox_amd import ops
    from test_quant_gpu import _record

    monkeypatch.setattr(ops.functional, "SKINNY_MAX_ROWS", 16)
    monkeypatch.setattr(ops.functional, "WIDE_MAX_ROWS", 64)
    monkeypatch.setattr(ops.functional, "TALL_MAX_ROWS", 256)
    calls = _record(monkeypatch)
    N, K = 144, 2112  # 66 units on 2 tiles: the rule splits K, so the launch uses the op's workspace
    assert ops._lib.call_ret("nsa_tall_gemm_ksplit", 65, N, K) > 1
    W, b = int_weight(N, K, False)[0].to(DEV), int_bias(N).to(DEV)
    assert _sums_below_2_24(int_x(256, K), W.cpu())

    def run(rows, w=W, bias=b):
        x = int_x(rows, K).to(DEV)
        del calls[:]
        return x, ops.decode_linear(x.view(rows, 1, K), w, bias, out_f32=True).view(rows, -1)

    for rows in (65, 256):
        x, y = run(rows)
        assert calls == ["nsa_tall_gemm"], calls
        assert torch.equal(y, linear_ref(x, W, None, b)[0].float())
    run(64)
    assert calls == ["nsa_wide_gemm"], calls
    for args in ((257,), (65, ops.quantize_rows_int8(W.float()), None), (65, ops.quantize_mxfp4(W.float()), None)):
        run(*args)
        assert calls and "nsa_tall_gemm" not in calls, calls
    monkeypatch.setattr(ops.functional, "TALL_MAX_ROWS", 64)
    run(65)
    assert calls and "nsa_tall_gemm" not in calls, calls
    # a split launch on few tiles, then one on 65 tiles (N > 8192) on the op's workspace: the partials of the
    # first lie where counters of the second would under a per-shape counter region
    monkeypatch.setattr(ops.functional, "TALL_MAX_ROWS", 256)
    Wb, bb = int_weight(8208, K, False)[0].to(DEV), int_bias(8208).to(DEV)
    assert ops._lib.call_ret("nsa_tall_gemm_ksplit", 65, 8208, K) > 1
    run(65)
    x, y = run(65, Wb, bb)
    assert calls == ["nsa_tall_gemm"], calls
    assert torch.equal(y, linear_ref(x, Wb, None, bb)[0].float())


def test_decoder_steps_80_rows_on_the_tall_kernel(kernels, monkeypatch):
    """80 rows through a two-layer model: the eager step's linears are ``nsa_tall_gemm`` launches, the captured
    graph draws the eager decoder's greedy tokens, and a second run of the same decoder repeats them."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.models import GPT, GPTConfig
    from nanosandbox_amd.runtime.decode import Decoder
    from test_quant_gpu import _record

    monkeypatch.setattr(ops.functional, "WIDE_MAX_ROWS", 64)
    monkeypatch.setattr(ops.functional, "TALL_MAX_ROWS", 256)
    torch.manual_seed(0)
    cfg = GPTConfig(block_size=64, vocab_size=128, n_layer=2, n_head=2, n_embd=128, dropout=0.0, bias=True)
    m = GPT(cfg).eval().to(DEV).set_compute_dtype(BF)
    idx = torch.randint(0, 128, (1, 5), device=DEV).expand(80, -1).contiguous()
    calls = _record(monkeypatch)
    eager = m.generate_cached(idx, 6, top_k=1, use_graph=False)
    assert calls.count("nsa_tall_gemm") >= 5 * (4 * cfg.n_layer + 1), calls  # 5 steps after the prefill's token
    dec = Decoder(m, 80, use_graph=True)
    try:
        first = m.generate_cached(idx, 6, top_k=1, decoder=dec)
        second = m.generate_cached(idx, 6, top_k=1, decoder=dec)
    finally:
        dec.release()
    assert dec.replays > 0
    assert torch.equal(first, eager) and torch.equal(second, first)
