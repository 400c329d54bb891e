"""int8 KV caches, CPU side: the cache-row quantizer's properties, the reference semantics of
``Decoder(kv_quantize="int8")`` (plain torch in fp32: what the ``_kv8`` kernels are tested
against) against a decoder written out here, the quantization error E_q on its own, and the
argument checks of the front ends."""

import math

import pytest
import torch
import torch.nn.functional as F

from nanosandbox_amd import ops
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder


def _model():  # tests/test_quant_gpu.py's, in fp32 on the CPU
    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval()


def _small(block_size=48):  # tests/test_quant_refs.py's
    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=block_size, vocab_size=97, n_layer=2, n_head=4, n_embd=64, dropout=0.0,
                         bias=True)).eval()


# ---------------------------------------------------------------------------- 1. quantizer

@pytest.mark.parametrize("shape,mul", [((2, 3, 5, 64), 1.0), ((1, 4, 77, 64), 30.0), ((1, 7, 16), 1e-3)])
def test_cache_quantizer_properties(shape, mul):
    torch.manual_seed(sum(shape))
    x = torch.randn(*shape) * mul
    x[0, ..., 1, :] = 0.0       # an all-zero row
    x[0, ..., 2, :] = -0.37     # a constant row
    qc = ops.quantize_cache_rows(x)
    assert isinstance(qc, ops.QuantCache) and isinstance(qc, tuple) and qc.shape == x.shape
    q, scale = qc
    assert q.dtype == torch.int8 and q.shape == x.shape and q.is_contiguous()
    assert scale.dtype == torch.float32 and scale.shape == x.shape[:-1] and scale.is_contiguous()
    assert int(q.min()) >= -127 and int(q.max()) <= 127
    absmax = x.abs().amax(dim=-1)
    nz = absmax > 0
    assert torch.equal(scale[nz], (absmax / torch.tensor(127.0))[nz])  # a true fp32 division
    assert bool((q[0, ..., 1, :] == 0).all()) and bool((scale[0, ..., 1] == 1.0).all())
    assert bool((q[0, ..., 2, :] == -127).all())
    assert bool((q.abs().amax(dim=-1)[nz] == 127).all())  # every non-zero row uses the full range
    # round to nearest: at most half a step away (the slack covers the fp32 division)
    deq = ops.dequantize_cache(qc)
    assert deq.dtype == torch.float32 and torch.equal(deq, q.float() * scale[..., None])
    err = (x.double() - q.double() * scale.double()[..., None]).abs()
    assert bool((err <= 0.5 * scale.double()[..., None] * (1 + 1e-4)).all())
    # the weight quantizer's rule, per cache row
    qw = ops.quantize_rows_int8(x.reshape(-1, shape[-1]))
    assert torch.equal(qw.q, q.reshape(-1, shape[-1])) and torch.equal(qw.scale, scale.reshape(-1))
    # bf16 input: quantized from its fp32 value
    qb = ops.quantize_cache_rows(x.bfloat16())
    qf = ops.quantize_cache_rows(x.bfloat16().float())
    assert torch.equal(qb.q, qf.q) and torch.equal(qb.scale, qf.scale)


def test_cache_quantizer_rounds_half_to_even():
    x = torch.zeros(1, 64)
    x[0, 0] = 127.0                                   # scale 1
    x[0, 1:7] = torch.tensor([0.5, 1.5, 2.5, -0.5, -1.5, -2.5])
    q = ops.quantize_cache_rows(x).q[0]
    assert q[:7].tolist() == [127, 0, 2, 2, 0, -2, -2]


# ---------------------------------------------------------------------------- 2. reference decoder

def _ln(x, ln):
    return F.layer_norm(x, (x.shape[-1],), ln.weight, ln.bias, 1e-5)


class _RefDecoder:
    """The int8-cache semantics written out for one sequence: the prompt attends over its own
    unquantized K / V and its rows are then stored quantized; a step quantizes the new K / V
    rows, appends them and attends over the dequantized rows 0 .. pos."""

    def __init__(self, m):
        self.m = m
        self.H = m.config.n_head
        self.k = [None] * m.config.n_layer  # per layer: (int8 [H, t, D], fp32 scale [H, t])
        self.v = [None] * m.config.n_layer

    @staticmethod
    def _quant(x):  # the stated rule, not ops.quantize_cache_rows
        amax = x.abs().amax(dim=-1, keepdim=True)
        scale = torch.where(amax > 0, amax / 127, torch.ones_like(amax))
        return torch.clamp(torch.round(x / scale), -127, 127), scale

    def _heads(self, t):  # [T, C] -> [H, T, D]
        return t.view(t.shape[0], self.H, -1).transpose(0, 1)

    def _block(self, i, x, prompt):
        blk = self.m.transformer.h[i]
        q, k, v = blk.attn.c_attn(_ln(x, blk.ln_1)).split(x.shape[-1], dim=-1)
        q, k, v = self._heads(q), self._heads(k), self._heads(v)
        D = q.shape[-1]
        kq, vq = self._quant(k), self._quant(v)
        if prompt:
            self.k[i], self.v[i] = kq, vq
            att = (q @ k.transpose(-2, -1)) / math.sqrt(D)
            T = x.shape[0]
            att = att.masked_fill(~torch.ones(T, T, dtype=torch.bool).tril(), float("-inf"))
            y = torch.softmax(att, dim=-1) @ v
        else:
            self.k[i] = tuple(torch.cat([a, b], dim=1) for a, b in zip(self.k[i], kq))
            self.v[i] = tuple(torch.cat([a, b], dim=1) for a, b in zip(self.v[i], vq))
            kd, vd = self.k[i][0] * self.k[i][1], self.v[i][0] * self.v[i][1]
            y = torch.softmax((q @ kd.transpose(-2, -1)) / math.sqrt(D), dim=-1) @ vd
        x = x + blk.attn.c_proj(y.transpose(0, 1).reshape(x.shape))
        return x + blk.mlp.c_proj(F.gelu(blk.mlp.c_fc(_ln(x, blk.ln_2))))

    def feed(self, toks, pos0, prompt):
        """toks [T] at positions pos0 .. -> the last position's logits [V]."""
        tr = self.m.transformer
        x = tr.wte(toks) + tr.wpe(torch.arange(pos0, pos0 + toks.numel()))
        for i in range(len(tr.h)):
            x = self._block(i, x, prompt)
        return self.m.lm_head(_ln(x[-1:], tr.ln_f))[0]


@pytest.mark.parametrize("lens", [None, [9, 30, 17]])
@torch.no_grad()
def test_kv8_decoder_is_the_reference(lens):
    """Shared position (lens None: every prompt 12 tokens) and per-row positions with unequal
    prompts.  fp32 on both sides; the tolerance covers batched against per-sequence matmuls."""
    m = _model()
    B, n_new = 3, 20
    torch.manual_seed(1)
    per_row = lens is not None
    L = lens or [12] * B
    idx = torch.randint(0, 512, (B, max(L) + n_new))
    dec = Decoder(m, B, use_graph=False, per_row=per_row, kv_quantize="int8")
    assert dec.kv_quantize == "int8" and all(isinstance(c, ops.QuantCache) for c in dec.kc + dec.vc)
    assert dec.kc[0].q.dtype == torch.int8 and dec.kc[0].q.shape == (B, 4, 256, 64)
    assert dec.kc[0].scale.dtype == torch.float32 and dec.kc[0].scale.shape == (B, 4, 256)
    T0 = max(L)
    lg = dec.prefill(idx[:, :T0], torch.tensor(L)) if per_row else dec.prefill(idx[:, :T0])
    refs = [_RefDecoder(m) for _ in range(B)]
    for b in range(B):
        want = refs[b].feed(idx[b, :L[b]], 0, True)
        assert torch.allclose(lg[b], want, atol=1e-4, rtol=1e-4), b
        # the prompt's rows are in the cache, quantized (the batched matmuls' last bits may move
        # a scale by an ulp and a value across a rounding boundary: at most one step)
        kq, ks = refs[b].k[1]
        assert int((dec.kc[1].q[b, :, :L[b]].float() - kq).abs().max()) <= 1
        assert torch.allclose(dec.kc[1].scale[b, :, :L[b]], ks[..., 0], rtol=1e-5, atol=0)
    for t in range(n_new):
        tok = torch.stack([idx[b, L[b] + t] for b in range(B)])
        lg = dec.step(tok)
        for b in range(B):
            want = refs[b].feed(tok[b:b + 1], L[b] + t, False)
            assert torch.allclose(lg[b], want, atol=1e-4, rtol=1e-4), (t, b)
    assert dec.positions == [n + n_new for n in L]
    dec.release()


@pytest.mark.parametrize("per_row", [False, True])
def test_kv8_append_form_equals_append_then_attend(per_row):
    torch.manual_seed(5)
    B, H, T, D = 3, 4, 40, 64
    C = H * D

    def caches():
        torch.manual_seed(6)
        return (ops.quantize_cache_rows(torch.randn(B, H, T, D)), ops.quantize_cache_rows(torch.randn(B, H, T, D)))

    qkv = torch.randn(B, 1, 3 * C)
    pos = torch.tensor([0, 17, 39]) if per_row else torch.tensor([23])
    (k1, v1), (k2, v2) = caches(), caches()
    y1 = ops.decode_attention(qkv, k1, v1, pos, H, append=True)
    ops.kv_append(qkv, k2, v2, pos)
    y2 = ops.decode_attention(qkv, k2, v2, pos, H, append=False)
    assert torch.equal(y1, y2)
    for a, b in ((k1, k2), (v1, v2)):
        assert torch.equal(a.q, b.q) and torch.equal(a.scale, b.scale)
    # the appended rows are the quantizer's, and the output is attention over the dequantized rows
    k, v = qkv.view(B, 3, H, D)[:, 1], qkv.view(B, 3, H, D)[:, 2]
    for b, p in enumerate(pos.tolist() * (1 if per_row else B)):
        want = ops.quantize_cache_rows(k[b])
        assert torch.equal(k1.q[b, :, p], want.q) and torch.equal(k1.scale[b, :, p], want.scale)
        kd, vd = ops.dequantize_cache(k1)[b, :, :p + 1], ops.dequantize_cache(v1)[b, :, :p + 1]
        att = torch.softmax(torch.einsum("hd,hkd->hk", qkv.view(B, 3, H, D)[b, 0], kd) / 8.0, dim=-1)
        assert torch.allclose(y1[b, 0].view(H, D), torch.einsum("hk,hkd->hd", att, vd), atol=1e-5, rtol=1e-5)
    # the prefill form with a host position
    qkv3 = torch.randn(B, 5, 3 * C)
    ops.kv_append(qkv3, k1, v1, None, 30)
    want = ops.quantize_cache_rows(qkv3.view(B, 5, 3, H, D)[:, :, 2].transpose(1, 2))
    assert torch.equal(v1.q[:, :, 30:35], want.q) and torch.equal(v1.scale[:, :, 30:35], want.scale)


# ---------------------------------------------------------------------------- 3. E_q

E_Q = 1.68e-3  # measured by test_kv8_quantization_error (its docstring)


def kv8_quantization_error(m, idx, T0):
    """max over steps T0 .. T-1 of |kv8 logits - full-forward logits|_F / |full-forward logits|_F,
    both in fp32 by the torch reference path."""
    with torch.no_grad():
        full = m.forward_logits(idx)
        dec = Decoder(m, idx.shape[0], use_graph=False, kv_quantize="int8")
        dec.prefill(idx[:, :T0])
        worst = 0.0
        for t in range(T0, idx.shape[1]):
            lg = dec.step(idx[:, t])
            worst = max(worst, ((lg - full[:, t]).norm() / full[:, t].norm()).item())
        dec.release()
    return worst


def test_kv8_quantization_error():
    """E_q: the int8 caches' own error, with nothing else in the way (fp32 weights, fp32
    arithmetic): steps 40 .. 71 of a B = 4 batch (seed 0) on the tiny model, relative Frobenius
    error of the logits against the full forward.  Measured: 1.677e-3 (E_Q; the figure is
    printed); asserted to stay within 1.5x of it.  Well below 1e-2."""
    m = _model()
    torch.manual_seed(0)
    idx = torch.randint(0, 512, (4, 72))
    e = kv8_quantization_error(m, idx, 40)
    print(f"E_q = {e:.4e}")
    assert 0 < e <= 1.5 * E_Q, e


# ---------------------------------------------------------------------------- 4. arguments

def test_kv_quantize_argument_checks(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    m = _small()
    idx = torch.randint(0, 97, (1, 10))
    with pytest.raises(ValueError):
        Decoder(m, 1, use_graph=False, kv_quantize="int4")
    with pytest.raises(ValueError):
        m.generate_cached(idx, 4, top_k=1, kv_quantize="fp8")
    with pytest.raises(ValueError):
        m.generate_batch([idx[0]], 4, top_k=1, kv_quantize="fp8")
    # prompt + new tokens past block_size: the recompute loop has no cache to quantize
    with pytest.raises(ValueError):
        m.generate_cached(idx, 48, top_k=1, kv_quantize="int8")
    with pytest.raises(ValueError):
        m.generate_batch([idx[0], idx[0, :3]], 48, top_k=1, kv_quantize="int8")
    # within block_size both run, alone and with int8 weights; greedy tokens in range
    y = m.generate_cached(idx, 20, top_k=1, kv_quantize="int8")
    assert y.shape == (1, 30) and torch.equal(y[:, :10], idx)
    ys = m.generate_batch([idx[0], idx[0, :3]], 20, top_k=1, kv_quantize="int8", quantize="int8")
    assert [t.numel() for t in ys] == [30, 23] and torch.equal(ys[1][:3], idx[0, :3])
    # a reused decoder of the other cache form is replaced by a temporary one
    dec = Decoder(m, 1, use_graph=False)
    y2 = m.generate_cached(idx, 20, top_k=1, kv_quantize="int8", decoder=dec)
    assert torch.equal(y2, y) and not isinstance(dec.kc[0], ops.QuantCache) and int(dec.pos) == 0
    dec.release()
    assert not [n for n, p in m.named_parameters() if hasattr(p, "compute")]

    args_model = dict(block_size=48, vocab_size=97, n_layer=2, n_head=4, n_embd=64, bias=True, dropout=0.0)
    (tmp_path / "prompt.txt").write_text("1,2,3")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    torch.save({"model": m.state_dict(), "model_args": args_model, "iter_num": 0, "best_val_loss": 0.0,
                "config": {}}, tmp_path / "ckpt.pt")
    args = [f"--out_dir={tmp_path}", "--device=cpu", "--num_samples=1", "--max_new_tokens=12",
            f"--start=FILE:{tmp_path / 'prompt.txt'}", "--top_k=1"]
    assert sample.SAMPLE_DEFAULTS["kv_quantize"] == ""
    with pytest.raises(ValueError):
        sample.main(args + ["--kv_quantize=int8", "--kv_cache=False"])
    with pytest.raises(ValueError):
        sample.main(args + ["--kv_quantize=int4"])
    got = sample.main(args + ["--kv_quantize=int8"])
    assert len(got) == 1 and len(got[0].split(",")) == 15 and got[0].startswith("1,2,3,")
    want = m.generate_cached(torch.tensor([[1, 2, 3]]), 12, top_k=1, kv_quantize="int8")
    assert got[0] == ",".join(map(str, want[0].tolist()))
    got = sample.main(args + ["--kv_quantize=int8", "--sample_batch=2", "--num_samples=2"])
    assert len(got) == 2 and got[0] == got[1] == ",".join(map(str, want[0].tolist()))
