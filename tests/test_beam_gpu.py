"""Beam search on the GPU: ``nsa_decode_attn_beam`` bit for bit against ``nsa_decode_attn_shared`` on gathered
caches, ``nsa_beam_step`` bit for bit against the rule, and ``generate_beam`` end to end."""

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.ops import _lib
from test_decode_attn_refs import BF, C, D, H, SCALE, peaked_bound, shared_ref
from test_decode_launches_gpu import PROMPT, _record, build_model

pytestmark = pytest.mark.gpu
DEV = "cuda"
TP, R = 192, 320
NEW = 12
# |beam score - GPT.score of the returned text|.  Measured on an MI355X at these sizes (2 / 4 / 8 rows, 9-token
# prompt, 12 new tokens): the plain decoder's ``logprobs=0`` sums lie at most SCORE_BASELINE from ``GPT.score`` on its own
# texts (bf16 summation order: one decode row against the batched forward); four times that is allowed.
SCORE_BASELINE = 0.025066  # worst of 2 / 4 / 8 rows x 12 seeds x 3 sampling settings: 0.022402, 0.022402, 0.025066
SCORE_BOUND = 4 * SCORE_BASELINE


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _attend(W, P, n, kind):
    """One beam launch with n slots in use -> (out, reference out, q, prompt caches, the gathered caches after the
    reference's append); the cache and guard assertions are made here."""
    g = torch.Generator().manual_seed(1000 * W + 10 * P + n)
    q = (3 * torch.randn(W, H, D, generator=g)).to(BF).to(DEV)
    kn, vn, pk, pv, kc, vc = (torch.randn(*s, generator=g).to(BF).to(DEV)
                              for s in [(W, H, D)] * 2 + [(1, H, TP, D)] * 2 + [(W, H, R, D)] * 2)
    src = {"identity": torch.arange(W)[:, None].expand(W, R), "other": ((torch.arange(W) + 1) % W)[:, None].expand(W, R),
           "random": torch.randint(0, W, (W, R), generator=g)}[kind].to(torch.int32).contiguous().to(DEV)
    slot = n - 1
    qkv = torch.stack([q, kn, vn], 1).reshape(W, 1, 3 * C).contiguous()
    plen, pos = torch.tensor([P], device=DEV), torch.tensor([P + slot], device=DEV)
    ar = torch.arange
    km, vm = (c[src.long()[:, None, :], ar(H, device=DEV)[None, :, None], ar(R, device=DEV)[None, None, :]]
              for c in (kc, vc))
    want = ops.decode_attention_shared(qkv, pk, pv, km, vm, plen, pos, H, append=True)
    kb, vb, pkb, pvb = kc.clone(), vc.clone(), pk.clone(), pv.clone()
    guard = torch.full((W + 2, C), float("nan"), device=DEV, dtype=BF)
    ws = torch.empty(W * H * (-(-TP // 128) + -(-R // 256)) * (4 + D), device=DEV)
    _lib.call("nsa_decode_attn_beam", *map(_lib.ptr, (qkv, pkb, pvb, kb, vb, src, plen, pos, ws, guard[1:-1])), W, H,
              TP, R, SCALE, 1, _lib.stream())
    assert bool(guard[0].isnan().all()) and bool(guard[-1].isnan().all())
    for cache, base, new in ((kb, kc, kn), (vb, vc, vn)):
        base = base.clone()
        base[:, :, slot] = new  # the append at (w, pos - P) and nothing else
        assert torch.equal(_bits(cache), _bits(base))
    assert torch.equal(_bits(pkb), _bits(pk)) and torch.equal(_bits(pvb), _bits(pv))
    return guard[1:-1], want.view(W, C), q, pk[0], pv[0], km, vm


@pytest.mark.parametrize("kind", ["identity", "other", "random"])
@pytest.mark.parametrize("n", [1, 256, 257])
@pytest.mark.parametrize("P", [1, 128, 129])
@pytest.mark.parametrize("W", [2, 5, 8])
def test_beam_attention_is_the_shared_kernel_on_gathered_caches(kernels, W, P, n, kind):
    out, want, *_ = _attend(W, P, n, kind)
    assert torch.equal(_bits(out), _bits(want))


def test_beam_attention_against_float64(kernels):
    W, P, n = 5, 129, 257
    out, _, q, pk, pv, km, vm = _attend(W, P, n, "random")
    ref, mag = shared_ref(q, pk, pv, km, vm, P, [P + n - 1] * W)
    err = (out.view(W, H, D).double() - ref).abs()
    assert bool((err <= peaked_bound(ref, mag)).all()), float((err / peaked_bound(ref, mag)).max())


def _state(W, n, kind, g):
    """A step's inputs and state on the CPU, values on a grid of 1/4 so that ties are everywhere."""
    lp = -torch.randint(0, 6, (W, W), generator=g).float().cumsum(1) / 4
    scores = -torch.randint(0, 8, (W,), generator=g).float() / 4
    done = (torch.rand(W, generator=g) < 0.4).to(torch.int32)
    ids = torch.randint(0, 12, (W, W), generator=g).to(torch.int32)
    if kind == "start":
        scores, done = torch.tensor([0.0] + [-float("inf")] * (W - 1)), torch.zeros(W, dtype=torch.int32)
        lp, ids = lp[:1].repeat(W, 1), ids[:1].repeat(W, 1)
    return dict(top_ids=ids, top_lp=lp, scores=scores, done=done,
                length=torch.randint(0, 9, (W,), generator=g).to(torch.int32), parent=torch.full((W,), -1, dtype=torch.int32),
                tok=torch.full((W, 1), -1), src=torch.randint(0, W, (W, R), generator=g).to(torch.int32),
                bp_parent=torch.full((R, W), -1, dtype=torch.int32), bp_token=torch.full((R, W), -1),
                n=torch.tensor([n], dtype=torch.int32), all_done=torch.tensor([-1], dtype=torch.int32))


@pytest.mark.parametrize("n", [0, 1, R - 1])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_beam_step_is_the_rule(kernels, W, n):
    g = torch.Generator().manual_seed(100 * W + n)
    for kind, stop in (("finished", 7), ("finished", None), ("start", 7), ("all done", 7)):
        want = _state(W, n, kind, g)
        if kind == "all done":
            want["done"].fill_(1)
        got = {k: v.to(DEV) for k, v in want.items()}
        ops.beam_step_(**want, stop_token=stop)
        ops.beam_step_(**got, stop_token=stop)
        for k in want:  # src and the back-pointers whole: what the step does not own is untouched
            a, b = got[k].cpu(), want[k]
            assert torch.equal(_bits(a), _bits(b)) if b.dtype == torch.float32 else torch.equal(a, b), (kind, stop, k)
        assert int(want["n"]) == n + 1 and int(want["all_done"]) == int(bool(want["done"].all()))


def test_beam_step_refuses_other_widths(kernels):
    s = {k: v.to(DEV) for k, v in _state(8, 0, "finished", torch.Generator().manual_seed(0)).items()}
    for W in (1, 9):
        with pytest.raises(RuntimeError, match="nsa_beam_step failed"):
            _lib.call("nsa_beam_step", *(_lib.ptr(s[k]) for k in ("top_ids", "top_lp", "scores", "done", "length", "parent",
                      "tok", "src", "bp_parent", "bp_token", "n", "all_done")), W, R, -1, _lib.stream())


@pytest.fixture(scope="module")
def model(kernels):
    return build_model()


@pytest.mark.parametrize("stop", [False, True], ids=["no-stop", "stop"])
@pytest.mark.parametrize("W", [2, 4, 8])
def test_generate_beam_end_to_end(model, W, stop):
    """Eager and captured runs agree to the bit, the hypotheses are distinct and ordered, and every score is the sum
    ``GPT.score`` gives the returned text: a wrong ancestor anywhere would break that.  Measured on an MI355X: see
    SCORE_BASELINE for the plain decoder's 0.025066; the beam scores' worst distance is 0.015160 at W = 2 and 4 and
    0.017333 at W = 8, eager and captured alike, against the bound of 0.100264."""
    T0 = PROMPT.numel()
    stop = int(model.generate_beam(PROMPT, NEW, W)[0][0][T0 + 2]) if stop else None
    outs, scores = model.generate_beam(PROMPT, NEW, W, stop_token=stop, use_graph=False)
    outs_g, scores_g = model.generate_beam(PROMPT, NEW, W, stop_token=stop, use_graph=True)
    assert [o.tolist() for o in outs] == [o.tolist() for o in outs_g] and torch.equal(_bits(scores), _bits(scores_g))
    assert len({tuple(o.tolist()) for o in outs}) == W and bool((scores[:-1] >= scores[1:]).all())
    if stop is not None:
        assert any(o.numel() < T0 + NEW and int(o[-1]) == stop for o in outs)
    worst = 0.0
    for o, s in zip(outs, scores.tolist()):
        assert o[:T0].tolist() == PROMPT.tolist() and (o.numel() == T0 + NEW or int(o[-1]) == stop)
        worst = max(worst, abs(s - float(model.score(o[None]).token[0, T0 - 1:].double().sum())))
    print(f"beam W {W} stop {stop}: worst |score - GPT.score| {worst:.6f} (bound {SCORE_BOUND:.6f})")
    assert worst <= SCORE_BOUND


def test_generate_beam_int8(model):
    with _record() as calls:
        outs, scores = model.generate_beam(PROMPT, NEW, 4, quantize="int8", use_graph=False)
    outs_g, scores_g = model.generate_beam(PROMPT, NEW, 4, quantize="int8", use_graph=True)
    assert [o.tolist() for o in outs] == [o.tolist() for o in outs_g] and torch.equal(_bits(scores), _bits(scores_g))
    linears = [c for c in calls if c.startswith(("nsa_skinny", "nsa_gemv"))]
    assert linears and all(c.endswith("_q8") for c in linears)
    assert "nsa_decode_attn_beam" in calls and "nsa_beam_step" in calls and "nsa_decode_attn_shared" not in calls
