"""``ops.quant_linear`` and ``Decoder(..., quantize_prefill=True)`` where no GPU is: the op's fallback is ``linear`` on
``dequantize(w)``, and the decoder without shadows of its block linears runs the same dequantized fp32 model."""

import pytest
import torch
import torch.nn.functional as F

from nanosandbox_amd import ops
from nanosandbox_amd.runtime.decode import Decoder
from test_quant_refs import _model, _quant_params

QUANTIZERS = {"int8": ops.quantize_rows_int8, "mxfp4": ops.quantize_mxfp4}


@pytest.mark.parametrize("quantize", ["int8", "mxfp4"])
@pytest.mark.parametrize("gelu", [False, True])
def test_quant_linear_is_linear_on_the_dequantized_weight(quantize, gelu):
    torch.manual_seed(3)
    x, b = torch.randn(2, 5, 96), torch.randn(40) * 0.1
    w = QUANTIZERS[quantize](torch.randn(40, 96) * 0.05)
    for bias in (None, b):
        ref = ops.linear(x, ops.dequantize(w), bias)
        ref = F.gelu(ref) if gelu else ref
        y = ops.quant_linear(x, w, bias, gelu=gelu)
        assert y.shape == (2, 5, 40) and y.dtype == torch.float32 and not y.requires_grad
        assert torch.equal(y, ref)
    with pytest.raises(TypeError):
        ops.quant_linear(x, torch.randn(40, 96))


@pytest.mark.parametrize("quantize", ["int8", "mxfp4"])
def test_cpu_decoder_without_shadows_runs_the_same_model(quantize):
    """Prefill and step logits of the flag-on decoder are those of the flag-off one (fp32: both read
    ``dequantize(w)``); no block linear carries a ``compute`` shadow while it lives, the tied table does, and
    ``release()`` leaves none; ``fits`` tells the two kinds apart; the front ends give the same greedy tokens."""
    m = _model()
    blocks, head = _quant_params(m)[:-1], m.lm_head.weight
    idx = torch.randint(0, 97, (3, 20))
    off = Decoder(m, 3, use_graph=False, quantize=quantize)
    with torch.no_grad():
        want = [off.prefill(idx[:, :8])] + [off.step(idx[:, t]).clone() for t in range(8, 14)]
    off.release()
    on = Decoder(m, 3, use_graph=False, quantize=quantize, quantize_prefill=True)
    assert not [p for p in blocks if hasattr(p, "compute")] and hasattr(head, "compute")
    assert on.fits(3, quantize=quantize, quantize_prefill=True) and not on.fits(3, quantize=quantize)
    assert off.fits(3, quantize=quantize) and not off.fits(3, quantize=quantize, quantize_prefill=True)
    with torch.no_grad():
        got = [on.prefill(idx[:, :8])] + [on.step(idx[:, t]).clone() for t in range(8, 14)]
    on.release()
    for t, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), t
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
    prompts = [idx[0, :3], idx[1, :5], idx[2, :9]]
    for a, b in zip(m.generate_batch(prompts, 6, top_k=1, quantize=quantize, quantize_prefill=True, batch_size=2),
                    m.generate_batch(prompts, 6, top_k=1, quantize=quantize, batch_size=2)):
        assert torch.equal(a, b)
    assert torch.equal(m.generate_cached(idx[:2, :5], 8, top_k=1, quantize=quantize, quantize_prefill=True),
                       m.generate_cached(idx[:2, :5], 8, top_k=1, quantize=quantize))
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]


def test_quantize_prefill_needs_quantize():
    m = _model()
    with pytest.raises(ValueError):
        Decoder(m, 2, quantize_prefill=True)
    with pytest.raises(ValueError):
        m.generate_cached(torch.zeros(1, 4, dtype=torch.long), 4, quantize_prefill=True)
    with pytest.raises(ValueError):
        m.generate_batch([torch.zeros(4, dtype=torch.long)], 4, quantize_prefill=True)
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]
