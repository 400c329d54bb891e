"""Log-probabilities on MI355X: ``nsa_token_logprobs`` against the float64 brute force within the bound
derived in ``test_logprob_refs`` (ids exactly the stable sort's), the decoder's records bit for bit
against the op on the logits the sampler was handed, in and out of the captured graph, the skip rule
at the stop token, at ``end`` and across ``admit``, ``GPT.score`` and one pass through every front end."""

import pytest
import torch

from test_logprob_refs import F64, NEG, adversarial_rows, brute, within
from test_penalty_gpu import V as TV
from test_penalty_gpu import _model, _prompts

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b):
    return all(torch.equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def _fresh(M, N):
    from nanosandbox_amd import ops

    return ops.LogProbs(torch.full((M,), float("nan"), device=DEV), torch.full((M, N), -7, dtype=torch.int32, device=DEV),
                        torch.full((M, N), float("nan"), device=DEV))


# the last four: both sides of the two thresholds between the kernel's three block forms
@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 50257, 50304, 53249, 14336, 14337, 57344,
                               57345])
def test_raw_op(kernels, V):
    from nanosandbox_amd import ops

    Mmax = 65
    L = adversarial_rows(V, Mmax)
    Lb = L.to(BF)
    g = torch.Generator().manual_seed(V)
    ids = torch.randint(0, V, (Mmax,), generator=g)
    ids[1], ids[2] = -1, V  # skipped rows
    ids[3] = V - 1          # the last column (the partial group's last)
    ref = {False: brute(L, ids, 8), True: brute(Lb.float(), ids, 8)}  # computed once, shared by every case
    Vpad = ops.lm_head_rows(V)
    ld = -(-V // 8) * 8 + 8
    strided = torch.full((Mmax, ld), 1e30, device=DEV)  # columns past V would win any maximum
    strided[:, :V] = L.to(DEV)
    flat = torch.full((1 + Mmax * ld,), 1e30, device=DEV)
    shifted = flat[1:].view(Mmax, ld)[:, :V]  # the base off by one element: the scalar form
    shifted.copy_(L)
    padded = torch.full((Mmax, Vpad), 1e30, device=DEV, dtype=BF)
    padded[:, :V] = Lb.to(DEV)
    layouts = [("contiguous", L.to(DEV), False), ("strided", strided[:, :V], False), ("shifted", shifted, False),
               ("bf16 ld=Vpad", padded, True)]
    worst = 0.0
    for M in (1, 3, 65):
        idm = ids[:M].to(DEV)
        ok = ((ids[:M] >= 0) & (ids[:M] < V))
        results = {}
        for name, lg, bf in layouts:
            lp64, ti, tl64 = (t[:M] for t in ref[bf])
            for N in (0, 1, 5, 8):
                out = _fresh(M, N)
                got = ops.token_logprobs(lg[:M], idm, top=N, V=V, out=out)
                again = ops.token_logprobs(lg[:M], idm, top=N, V=V, out=_fresh(M, N))
                assert _same(got, again), (V, M, name, N)  # two launches: the same bits
                tok, tid, top = got.token.cpu(), got.top_ids.cpu(), got.top.cpu()
                assert bool(torch.isnan(tok[~ok]).all()) and bool((tid[~ok] == -7).all()), (V, M, name, N)
                assert bool(torch.isnan(top[~ok]).all()), (V, M, name, N)  # skipped rows keep their sentinels
                assert bool(within(tok[ok], lp64[ok], V).all()), (V, M, name, N, tok[ok], lp64[ok])
                assert torch.equal(tid[ok], ti[ok][:, :N]), (V, M, name, N)  # exactly the stable sort's
                assert bool(within(top[ok], tl64[ok][:, :N], V).all()), (V, M, name, N)
                fin = ok & torch.isfinite(lp64)
                if fin.any():
                    worst = max(worst, float(((tok[fin].to(F64) - lp64[fin]).abs()
                                              / (2.0 ** -24 * (2 * lp64[fin].abs() + 1))).max()))
                if N == 8:
                    results[name] = got
                    if V < 8:
                        assert bool((tid[ok][:, V:] == -1).all()) and bool((top[ok][:, V:] == NEG).all())
                else:  # the drawn token's log-probability does not depend on N
                    assert torch.equal(_bits(got.token), _bits(ops.token_logprobs(lg[:M], idm, top=8, V=V).token))
        # one summation order: the vector and the scalar form, any row stride
        assert _same(results["contiguous"], results["strided"]) and _same(results["contiguous"], results["shifted"])
    print(f"V={V}: worst |error| = {worst:.2f} x 2^-24 (2 |lp| + 1)")


def _decoder(model, B, N, graph, **kw):
    from nanosandbox_amd.runtime.decode import Decoder

    dec = Decoder(model, B, per_row=True, logprobs=N, use_graph=graph, **kw)
    dec.salt = 4242  # the same sampling stream in every decoder of a test
    return dec


def _records(dec):
    return [t.clone() for t in (dec.lp, dec.top_ids, dec.top_lp)]


def _check_draw(dec, logits, rows=None):
    """``lp`` / ``top_*`` at every row's position are the op on (the sampler's logits, the drawn token)."""
    from nanosandbox_amd import ops

    want = ops.token_logprobs(logits.contiguous(), dec.tok.view(-1), top=dec.logprobs, V=TV)
    pos = dec.pos.expand(dec.B).tolist()
    for b in (range(dec.B) if rows is None else rows):
        p = pos[b]
        assert _same((dec.lp[b, p], dec.top_ids[b, p], dec.top_lp[b, p]), (want.token[b], want.top_ids[b], want.top[b])), b
        assert int(dec.lp_last[b]) == p and bool(torch.isfinite(dec.lp[b, p]))


def test_decoder_records_the_op_on_the_samplers_logits(kernels):
    from nanosandbox_amd.runtime.decode import Decoder, _right_pad

    model = _model()
    prompts = _prompts([5, 9, 3])
    N, steps, samp = 2, 12, (0.9, 40)
    eager = _decoder(model, 3, N, False)
    logits = eager.prefill(*_right_pad(prompts, DEV))
    kept = logits.clone()
    eager.sample_into(logits, *samp)
    _check_draw(eager, kept)
    for _ in range(steps):
        logits = eager._step_impl()
        kept = logits.clone()
        eager.sample_into(logits, *samp)
        _check_draw(eager, kept)
    # the captured graph: the same ids and the same records, bit for bit
    graph = _decoder(model, 3, N, True)
    graph.sample_into(graph.prefill(*_right_pad(prompts, DEV)), *samp)
    graph.run(steps, *samp)
    assert graph.use_graph and any("lp" in k for k in graph.sgraphs)
    assert torch.equal(graph.gen, eager.gen) and _same(_records(graph), _records(eager))
    assert torch.equal(graph.lp_last, eager.lp_last)
    for b, p in enumerate(prompts):  # exactly the new positions are recorded
        rec = torch.isfinite(graph.lp[b])
        assert rec.nonzero().view(-1).tolist() == list(range(p.numel(), p.numel() + steps + 1))
    # ... and with logprobs off the ids are the same
    plain = Decoder(model, 3, per_row=True)
    plain.salt = 4242
    plain.sample_into(plain.prefill(*_right_pad(prompts, DEV)), *samp)
    plain.run(steps, *samp)
    assert plain.lp is None and not any("lp" in k for k in plain.sgraphs)
    assert torch.equal(plain.gen, graph.gen)
    for d in (eager, graph, plain):
        d.release()


def test_a_finished_row_records_its_last_token_and_nothing_after(kernels):
    from nanosandbox_amd.runtime.decode import _right_pad

    model = _model()
    prompts = _prompts([4, 7, 6])
    N, samp = 3, (1.0, 50)
    probe = _decoder(model, 3, N, True)
    probe.sample_into(probe.prefill(*_right_pad(prompts, DEV)), *samp)
    probe.run(6, *samp)
    stop = int(probe.gen[1, 7 + 4])  # what row 1 draws fifth
    first = int((probe.gen[1, 7:7 + 5] == stop).nonzero()[0])  # ... unless it drew it earlier
    probe.release()
    dec = _decoder(model, 3, N, True)
    dec.sample_into(dec.prefill(*_right_pad(prompts, DEV)), *samp, stop)
    dec.run(6, *samp, stop)
    assert int(dec.done[1]) == 1 and int(dec.pos[1]) == 7 + first
    assert int(dec.gen[1, 7 + first]) == stop and bool(torch.isfinite(dec.lp[1, 7 + first]))  # the stop token is recorded
    assert int(dec.top_ids[1, 7 + first, 0]) >= 0 and bool(torch.isnan(dec.lp[1, 7 + first + 1:]).all())
    before = [t[1].clone() for t in _records(dec)]
    live = [b for b in (0, 2) if not int(dec.done[b])]
    seen = int(torch.isfinite(dec.lp[live]).sum())
    for _ in range(20):  # the graph itself, whatever run() would poll
        next(iter(dec.sgraphs.values())).replay()
    assert _same([t[1] for t in _records(dec)], before)  # the finished row: bit for bit unchanged
    live = [b for b in live if not int(dec.done[b])] or live
    assert int(torch.isfinite(dec.lp[live]).sum()) > seen  # the others kept recording
    dec.release()


def test_queue_rows_end_and_admit(kernels):
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import _right_pad

    model = _model()
    prompts = _prompts([5, 8, 6])
    N, samp = 2, (0.8, 30)
    dec = _decoder(model, 3, N, True)
    dec._queue_state()
    dec.key.copy_(torch.tensor([7, 8, 9], device=DEV))
    dec.end.copy_(torch.tensor([5 + 3, 8 + 40, 6 + 40], device=DEV))  # row 0: 4 new tokens, at positions 5 .. 8
    dec.sample_into(dec.prefill(*_right_pad(prompts, DEV)), *samp, queue=True)
    dec.run(8, *samp, queue=True)
    assert dec.done.tolist() == [1, 0, 0] and int(dec.pos[0]) == 8
    assert torch.isfinite(dec.lp[0]).nonzero().view(-1).tolist() == [5, 6, 7, 8]  # the token at ``end`` included
    before = [t.clone() for t in _records(dec)]
    dec.run(20, *samp, queue=True)
    after = _records(dec)
    assert _same([t[0] for t in after], [t[0] for t in before])
    assert int(torch.isfinite(after[0][1:]).sum()) == int(torch.isfinite(before[0][1:]).sum()) + 40
    # admit a new prompt into row 0: it records again from its new start, the others are untouched
    new = _prompts([11], seed=9)
    dec.end[0] = 11 + 5
    logits = dec.admit([0], *_right_pad(new, DEV))
    assert int(dec.lp_last[0]) == -1 and bool(torch.isnan(dec.lp[0]).all()) and bool((dec.top_ids[0] == -1).all())
    dec.sample_admitted([0], logits, *samp)
    want = ops.token_logprobs(logits.float().contiguous(), dec.tok[:1].view(-1), top=N, V=TV)
    assert _same((dec.lp[0, 11], dec.top_ids[0, 11], dec.top_lp[0, 11]), (want.token[0], want.top_ids[0], want.top[0]))
    assert torch.isfinite(dec.lp[0]).nonzero().view(-1).tolist() == [11]
    now = _records(dec)
    assert _same([t[1:] for t in now], [t[1:] for t in after])
    dec.run(3, *samp, queue=True)
    assert torch.isfinite(dec.lp[0]).nonzero().view(-1).tolist() == [11, 12, 13, 14]
    dec.release()
    # the queue's front end harvests a request's records with its ids
    torch.manual_seed(5)
    reqs = _prompts([4, 9, 5, 7, 3], seed=3)
    outs, recs = model.generate_batch(reqs, [6, 3, 9, 4, 5], temperature=0.8, top_k=30, batch_size=2, logprobs=1)
    torch.manual_seed(5)
    plain = model.generate_batch(reqs, [6, 3, 9, 4, 5], temperature=0.8, top_k=30, batch_size=2)
    for p, o, w, r, n in zip(reqs, outs, plain, recs, [6, 3, 9, 4, 5]):
        assert torch.equal(o, w) and r.token.shape == (n,) and r.top_ids.shape == (n, 1)
        assert bool(torch.isfinite(r.token).all()) and bool((r.top[:, 0] >= r.token).all())


def test_score_on_the_gpu(kernels):
    from nanosandbox_amd import ops

    model = _model()
    g = torch.Generator().manual_seed(12)
    idx = torch.randint(0, TV, (3, 33), generator=g).to(DEV)
    lens = torch.tensor([33, 20, 2])
    model.SCORE_CHUNK_ROWS = 40  # 96 rows: two whole chunks and a short one
    s = model.score(idx, lengths=lens, top=4)
    logits = model.forward_logits(idx)[:, :-1].to(BF).float().reshape(96, TV)  # rounded through bf16
    ids = idx[:, 1:].reshape(-1)
    lp64, ti, tl64 = brute(logits.cpu(), ids.cpu(), 4)
    op = ops.token_logprobs(logits, ids, top=4)
    given = (torch.arange(1, 33)[None, :] < lens[:, None]).view(-1)
    tok, tid, top = s.token.view(-1).cpu(), s.top_ids.view(96, 4).cpu(), s.top.view(96, 4).cpu()
    err = (tok[given].to(F64) - lp64[given]).abs().max()
    print(f"score: worst |error| against float64 = {float(err):.3e}; against the op: "
          f"{float((tok[given] - op.token.cpu()[given]).abs().max()):.3e}")
    assert bool(within(tok[given], lp64[given], TV).all())
    assert torch.equal(tid[given], ti[given]) and bool(within(top[given], tl64[given], TV).all())
    assert bool(torch.isnan(tok[~given]).all()) and bool((tid[~given] == -1).all())  # the skipped tail
    assert int(given.sum()) == 32 + 19 + 1
    ppl = s.perplexity().cpu()
    assert abs(float(ppl[1]) - float(torch.exp(-lp64.view(3, 32)[1, :19].mean()))) < 1e-3 * float(ppl[1])


FRONT_ENDS = {
    "shared_prompt": dict(shared_prompt=True),
    "shared_prefix": dict(shared_prefix=True),
    "int8 weights": dict(quantize="int8"),
    "int8 caches": dict(kv_quantize="int8"),
    "penalties": dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2),
}


@pytest.mark.parametrize("mode", list(FRONT_ENDS))
def test_front_end_records_equal_the_op_on_each_steps_logits(kernels, monkeypatch, mode):
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder

    model = _model()
    if mode == "shared_prompt":
        prompts = _prompts([6]) * 3
    elif mode == "shared_prefix":
        head = _prompts([5])[0]
        prompts = [torch.cat([head, t]) for t in _prompts([2, 4, 3], seed=8)]
    else:
        prompts = _prompts([4, 7, 5])
    calls = []
    sample_into = Decoder.sample_into

    def spy(self, logits, *a, **kw):
        kept = logits.float().contiguous().clone()
        sample_into(self, logits, *a, **kw)
        calls.append((kept, self.tok.view(-1).clone(), self.pos.expand(self.B).tolist()))

    monkeypatch.setattr(Decoder, "sample_into", spy)
    n = 6
    outs, recs = model.generate_batch(prompts, n, temperature=0.9, top_k=40, use_graph=False, logprobs=2,
                                      **FRONT_ENDS[mode])
    assert len(calls) == n
    for kept, tok, pos in calls:
        want = ops.token_logprobs(kept, tok, top=2, V=TV)
        for b, p in enumerate(prompts):
            i = pos[b] - p.numel()
            assert int(outs[b][pos[b]]) == int(tok[b])
            assert _same((recs[b].token[i], recs[b].top_ids[i], recs[b].top[i]),
                         (want.token[b], want.top_ids[b], want.top[b])), (mode, b, i)
    for r in recs:
        assert r.token.shape == (n,) and bool(torch.isfinite(r.token).all())
