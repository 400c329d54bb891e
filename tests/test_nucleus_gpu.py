"""Nucleus (top-p) and min-p sampling on MI355X: the kept set of ``nsa_sample_filtered``
(reported through ``stats``), its draws and the graph-replayed decode step, against the
float64 reference and fixtures of tests/test_nucleus_refs.py."""

import pytest
import torch

from test_nucleus_refs import FIXTURE_IDS, FIXTURES, V64_SETTINGS, check_stats, logits_of, ref_of

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _setting(name):
    _, lname, T, k, p, mp, _ = FIXTURES[FIXTURE_IDS.index(name)]
    return logits_of(lname), T, k, p, mp


def _bufs(R, width):
    tok = torch.full((R, 1), -1, dtype=torch.int64, device=DEV)
    gen = torch.full((R, width), -1, dtype=torch.int64, device=DEV)
    stats = torch.full((R, 2), -1, dtype=torch.int32, device=DEV)
    return tok, gen, stats


@pytest.mark.parametrize("per_row", [False, True], ids=["shared", "rows"])
@pytest.mark.parametrize("name", FIXTURE_IDS)
def test_kept_set(kernels, name, per_row):
    from nanosandbox_amd import ops

    l, T, k, p, mp = _setting(name)
    R = 8
    logits = l.to(DEV).expand(R, -1).contiguous()
    tok, gen, stats = _bufs(R, 4)
    pos = torch.full((R if per_row else 1,), 2, dtype=torch.int64, device=DEV)
    ops.sample_topk_(logits, T, k, 31, pos, tok, gen, top_p=p, min_p=mp, stats=stats)
    st = stats.cpu()
    check_stats(name, int(st[0, 0]), int(st[0, 1]))
    assert bool((st == st[0]).all())  # all rows agree
    assert torch.equal(gen[:, 2], tok[:, 0]) and int(tok.min()) >= 0


@pytest.mark.parametrize("name", FIXTURE_IDS)
def test_support(kernels, name):
    from nanosandbox_amd import ops

    l, T, k, p, mp = _setting(name)
    r = ref_of(name)
    R = 64
    logits = l.to(DEV).expand(R, -1).contiguous()
    tok, gen, stats = _bufs(R, 4)
    for step in range(4):
        ops.sample_topk_(logits, T, k, 77, torch.tensor([step], dtype=torch.int64, device=DEV), tok, gen,
                         top_p=p, min_p=mp, stats=stats)
        assert torch.equal(gen[:, step], tok[:, 0])
    low = stats[:, 1].cpu().view(torch.float32)
    assert bool((low == low[0]).all())
    drawn = l[gen.cpu().view(-1)]
    assert bool((drawn >= low[0]).all()), (float(drawn.min()), float(low[0]))
    if r.n == 1:
        assert bool((gen == int(l.argmax())).all())


@pytest.mark.parametrize("name", [f[0] for f in V64_SETTINGS])
def test_distribution(kernels, name):
    """The shape of test_device_sampling_distribution: 32k draws over 64 ids, total
    variation against the reference probabilities < 0.03 (sampling noise <= 0.018)."""
    from nanosandbox_amd import ops

    l, T, k, p, mp = _setting(name)
    r = ref_of(name)
    V, R = 64, 4096
    logits = l.to(DEV).expand(R, V).contiguous()
    tok, gen, _ = _bufs(R, 8)
    for step in range(8):
        ops.sample_topk_(logits, T, k, 1234, torch.tensor([step], dtype=torch.int64, device=DEV), tok, gen,
                         top_p=p, min_p=mp)
        assert torch.equal(gen[:, step], tok[:, 0])
    counts = torch.bincount(gen.view(-1), minlength=V).cpu().double()
    assert counts[~r.keep].sum() == 0  # nothing outside the kept set
    tv = 0.5 * (counts / counts.sum() - r.p).abs().sum().item()
    print(f"{name}: total variation {tv:.4f}")
    assert tv < 0.03, tv


def test_per_row_contract(kernels):
    from nanosandbox_amd import ops

    l, T, k, p, mp = _setting("v64-kpm")  # kept = 1: every live row draws the arg-max
    am = int(l.argmax())
    B = 4
    logits = l.to(DEV).expand(B, -1).contiguous()
    positions = [3, 9, 9, 40]
    pos = torch.tensor(positions, device=DEV, dtype=torch.int64)
    done = torch.tensor([0, 0, 1, 0], device=DEV, dtype=torch.int64)
    tok, gen, stats = _bufs(B, 48)
    tok.fill_(777)
    ops.sample_topk_(logits, T, k, 99, pos, tok, gen, stop_token=am, done=done, top_p=p, min_p=mp, stats=stats)
    want = torch.full((B, 48), -1, device=DEV, dtype=torch.int64)
    for b in (0, 1, 3):
        want[b, positions[b]] = am
    assert tok.view(-1).tolist() == [am, am, 777, am] and torch.equal(gen, want)
    assert stats[2].tolist() == [-1, -1] and stats[0].tolist() == [1, int(l.max().view(torch.int32))]
    assert done.tolist() == [1, 1, 1, 1]  # a row that draws the stop token is finished
    # another stop token: nobody finishes
    done2 = torch.zeros(B, device=DEV, dtype=torch.int64)
    ops.sample_topk_(logits, T, k, 99, pos, tok, gen, stop_token=(am + 1) % 64, done=done2, top_p=p, min_p=mp)
    assert done2.tolist() == [0, 0, 0, 0]
    # equal positions: the per-row draw is the shared-position draw, bit for bit
    for name in ("v64-p", "zipf1.3-p", "randn-p"):
        l, T, k, p, mp = _setting(name)
        logits = l.to(DEV).expand(16, -1).contiguous()
        t1, g1, _ = _bufs(16, 12)
        t2, g2, _ = _bufs(16, 12)
        ops.sample_topk_(logits, T, k, 99, torch.full((16,), 9, device=DEV, dtype=torch.int64), t1, g1,
                         top_p=p, min_p=mp)
        ops.sample_topk_(logits, T, k, 99, torch.tensor([9], device=DEV, dtype=torch.int64), t2, g2, top_p=p, min_p=mp)
        assert torch.equal(t1, t2) and torch.equal(g1, g2)
        assert len(set(t1.view(-1).tolist())) > 1  # rows draw from their own streams


@pytest.mark.parametrize("V,top_k", [(50304, 200), (64, None), (63, 5), (50304, 2000)])
def test_no_change_at_defaults(kernels, V, top_k):
    """top_p = 1, min_p = 0 through the new entry point: the ids of the top-k sampler."""
    from nanosandbox_amd import ops

    torch.manual_seed(V)
    R = 32
    logits = (torch.randn(R, V) * 2).to(DEV)
    for per_row in (False, True):
        pos = torch.full((R if per_row else 1,), 5, dtype=torch.int64, device=DEV)
        t1, g1, _ = _bufs(R, 8)
        t2, g2, stats = _bufs(R, 8)
        ops.sample_topk_(logits, 0.8, top_k, 4321, pos, t1, g1)
        ops.sample_topk_(logits, 0.8, top_k, 4321, pos, t2, g2, top_p=1.0, min_p=0.0, stats=stats)
        assert torch.equal(t1, t2) and torch.equal(g1, g2)
        assert stats[:, 0].tolist() == [top_k or V] * R  # randn rows: no ties at the k-th logit


def test_c_entry_rejects_out_of_range(kernels):
    from nanosandbox_amd.ops import _lib

    logits = torch.zeros(1, 64, device=DEV)
    tok, gen, _ = _bufs(1, 2)
    pos = torch.zeros(1, dtype=torch.int64, device=DEV)
    for top_p, min_p in ((0.0, 0.0), (1.5, 0.0), (0.9, 1.0), (0.9, -0.1), (float("nan"), 0.0)):
        with pytest.raises(RuntimeError, match="hipError 1"):
            _lib.call("nsa_sample_filtered", _lib.ptr(logits), 1, 64, 64, 1.0, 0, top_p, min_p, 1, None, _lib.ptr(pos),
                      0, _lib.ptr(tok), _lib.ptr(gen), 2, -1, None, None, _lib.stream())
    assert int(tok) == -1


def _model():
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


def test_graph_decode_matches_eager(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    idx = torch.randint(0, 512, (2, 16), device=DEV)
    outs = {}
    for g in (True, False):
        torch.manual_seed(3)  # the draw is a counter hash of the salt drawn here
        outs[g] = m.generate_cached(idx, 40, temperature=0.9, top_k=0, top_p=0.9, use_graph=g)
    assert outs[True].shape == (2, 56) and torch.equal(outs[True], outs[False])
    assert len(set(outs[True][0, 16:].tolist())) > 4  # sampling, not a constant

    prompts = [torch.randint(0, 512, (n,), device=DEV) for n in (5, 40, 33)]
    torch.manual_seed(4)
    free = m.generate_batch(prompts, 30, top_p=0.9, min_p=0.05, use_graph=False)
    stop = int(free[1][40 + 6])  # the 7th new token of the second row
    outs = {}
    for g in (True, False):
        torch.manual_seed(4)
        outs[g] = m.generate_batch(prompts, 30, top_p=0.9, min_p=0.05, stop_token=stop, use_graph=g)
    assert all(torch.equal(a, b) for a, b in zip(outs[True], outs[False]))
    assert outs[True][1].numel() <= 40 + 7 and int(outs[True][1][-1]) == stop

    # a second nucleus setting on one decoder: a second graph, and both stay usable
    torch.manual_seed(5)  # a decoder draws its salt where it is built: the same one for both
    dec = Decoder(m, 2, max_len=256, use_graph=True)
    torch.manual_seed(5)
    eager = Decoder(m, 2, max_len=256, use_graph=False)
    try:
        runs = []
        for top_p in (0.9, 0.5, 0.9, 0.5):
            torch.manual_seed(6)
            runs.append(m.generate_cached(idx, 24, top_k=0, top_p=top_p, decoder=dec))
        assert len(dec.sgraphs) == 2
        assert torch.equal(runs[0], runs[2]) and torch.equal(runs[1], runs[3])
        for top_p, got in zip((0.9, 0.5), runs):
            torch.manual_seed(6)
            assert torch.equal(got, m.generate_cached(idx, 24, top_k=0, top_p=top_p, decoder=eager))
        assert not torch.equal(runs[0], runs[1])
        # the old arguments still key (and capture) what they did
        m.generate_cached(idx, 8, top_k=5, decoder=dec)
        assert (1.0, 5) in dec.sgraphs and len(dec.sgraphs) == 3
    finally:
        dec.release()
        eager.release()
