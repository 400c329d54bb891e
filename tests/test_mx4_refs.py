"""MXFP4 weight-only decoding on the CPU: the format (``ops.MxWeight``), the quantizer (``ops.quantize_mxfp4``)
and ``Decoder(quantize="mxfp4")``, which there runs the dequantized model in fp32."""

import copy

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.runtime.decode import Decoder
from test_quant_refs import _model, _quant_params

BF = torch.bfloat16
TABLE = [0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0]
TABLE = torch.tensor(TABLE + [-v for v in TABLE])


def _dequantized_copy(m):
    m2 = copy.deepcopy(m)
    with torch.no_grad():
        for p in _quant_params(m2):
            p.copy_(ops.dequantize(ops.quantize_mxfp4(p)))
    return m2


def test_codes_and_nibble_order():
    """The 16 codes decode to the table at scale byte 127 and 2^(e - 127) elsewhere; element k sits in byte
    k // 2, even k in the low nibble (a row whose even and odd elements differ)."""
    codes = torch.arange(16, dtype=torch.uint8).repeat(2)                  # k -> code k % 16
    q = (codes[0::2] | (codes[1::2] << 4)).view(1, 16)
    for e in (127, 124, 130):
        dq = ops.dequantize(ops.MxWeight(q, torch.tensor([[e]], dtype=torch.uint8)))
        assert dq.dtype == torch.float32 and torch.equal(dq.view(-1), TABLE.repeat(2) * 2.0 ** (e - 127))
    w = torch.zeros(1, 64)
    w[0, 0::2], w[0, 1::2] = 1.0, -6.0                                     # even k: code 2; odd k: code 8 + 7
    mw = ops.quantize_mxfp4(w)
    assert mw.shape == (1, 64) and mw.q.dtype == mw.scale.dtype == torch.uint8 and mw.q.shape == (1, 32)
    assert bool((mw.q == (2 | (15 << 4))).all()) and mw.scale.tolist() == [[127, 127]]
    assert torch.equal(ops.dequantize(mw), w)


@pytest.mark.parametrize("mul", [1.0, 2.0 ** -100, 2.0 ** 100])  # about 1e-30 and 1e30, the ties kept exact
def test_quantizer_properties(mul):
    """Every value exact in bf16 (the exponent clamp holds at both ends); a zero block; quantize(dequantize)
    reproduces codes and bytes; every element is the nearest of the representable values at its block's scale,
    by brute force over the table, ties to the even code."""
    torch.manual_seed(7)
    w = torch.randn(24, 160) * 0.05
    w[3, 32:64] = 0.0
    w[5, :32] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0, 6.0] * 4) * 0.125   # every tie, amax 6
    w = w * mul
    w[7, :32], w[8, :32] = 1e-38, -3e38                                     # bytes -2 and 252 before the clamp
    mw = ops.quantize_mxfp4(w)
    assert int(mw.scale[7, 0]) == 2 and int(mw.scale[8, 0]) == 252
    dq = ops.dequantize(mw)
    assert torch.equal(dq.to(BF).float(), dq)
    assert 2 <= int(mw.scale.min()) and int(mw.scale.max()) <= 252
    assert int(mw.scale[3, 1]) == 127 and bool((mw.q[3, 16:32] == 0).all())
    again = ops.quantize_mxfp4(dq)
    assert torch.equal(again.q, mw.q) and torch.equal(again.scale, mw.scale)
    code = torch.stack((mw.q & 15, mw.q >> 4), dim=2).view(24, 160).long()
    scale = torch.exp2(mw.scale.double() - 127).repeat_interleave(32, dim=1)
    a = w.double() / scale                                                  # exact: a power of two
    dist = (a[..., None] - TABLE.double()).abs()                            # [N, K, 16]
    best = dist.min(dim=-1).values
    assert torch.equal(dist.gather(-1, code[..., None])[..., 0], best)      # a nearest value (6 when beyond it)
    tie = (dist == best[..., None]).sum(-1) > 1
    assert bool(tie[5, :7].all()) and bool((code[tie & (a != 0)] % 2 == 0).all())
    assert bool((code[a == 0] == 0).all())


def test_decoder_runs_the_dequantized_model():
    """quantize="mxfp4" on the CPU equals the plain decoder on a deep copy holding the dequantized weights:
    logits equal in fp32 and the same greedy tokens; no ``compute`` attribute is left behind.  Recorded, not
    gated: relative logits error of this tiny random model against the unquantized one 0.1573 (OCP scale rule;
    the rejected no-clipping rule 0.1658; per-row int8 0.0084).  No trained snapshot: loss unmeasured."""
    m = _model()
    m2 = _dequantized_copy(m)
    idx = torch.randint(0, 97, (3, 20))
    dec, ref = Decoder(m, 3, use_graph=False, quantize="mxfp4"), Decoder(m2, 3, use_graph=False)
    with torch.no_grad():
        assert torch.equal(dec.prefill(idx[:, :8]), ref.prefill(idx[:, :8]))
        for t in range(8, 20):
            assert torch.equal(dec.step(idx[:, t]), ref.step(idx[:, t])), t
    dec.release(), ref.release()
    assert torch.equal(m.generate_cached(idx[:2, :5], 30, top_k=1, quantize="mxfp4"), m2.generate(idx[:2, :5], 30, top_k=1))
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
    with pytest.raises(ValueError):
        Decoder(m, 3, quantize="fp4")
    with pytest.raises(ValueError):
        Decoder(m, 3, quantize="int4")
