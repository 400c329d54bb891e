"""Repetition, presence and frequency penalties on MI355X: the penalised sampler
(``nsa_sample_penalized``) bit for bit against the plain entry points on logits penalised by
``ops.penalize_logits`` on the CPU, the histogram kernel against ``torch.bincount``, the decoder's
count table against the histograms of the rows' texts, and the front ends end to end."""

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
V = 512
RP, PP, FP = 1.3, 0.5, 0.2
PEN = dict(repetition_penalty=RP, presence_penalty=PP, frequency_penalty=FP)


def _model():
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=V, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False))
    return m.eval().to(DEV).set_compute_dtype(BF)


def _prompts(lens, seed=6):
    g = torch.Generator().manual_seed(seed)  # host RNG: the same prompts everywhere
    return [torch.randint(0, V, (k,), generator=g).to(DEV) for k in lens]


def _distinct(lens, seed=6):
    """Prompts whose ids are all different within a prompt."""
    g = torch.Generator().manual_seed(seed)
    return [torch.randperm(V, generator=g)[:k].to(DEV) for k in lens]


def _hist(ids, width=V):
    return torch.bincount(ids.view(-1).cpu(), minlength=width).to(torch.int32)


SETTINGS = [dict(top_k=200), dict(top_k=200, stats=True), dict(top_k=2000), dict(top_k=2000, stats=True),
            dict(top_k=None), dict(top_k=None, stats=True), dict(top_k=0, top_p=0.9, stats=True),
            dict(top_k=50, min_p=0.05, stats=True)]


@pytest.mark.parametrize("req", [False, True])
@pytest.mark.parametrize("Vs", [50304, 50257, 97])
def test_penalised_sampler_is_the_plain_one_on_penalised_logits(kernels, Vs, req):
    from nanosandbox_amd import ops

    g = torch.Generator().manual_seed(Vs + req)
    B, G, T = 4, 16, 0.8
    W = -(-Vs // 4) * 4  # the table's row: the vocabulary rounded up to 4
    L = torch.randn(B, Vs, generator=g) * 3.0
    L[0, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    C = torch.tensor([0, 0, 0, 1, 2, 9], dtype=torch.int32)[torch.randint(0, 6, (B, W), generator=g)]
    C[0, :4] = torch.tensor([1, 1, 0, 0], dtype=torch.int32)  # signed zeros, seen and unseen
    C[1] = 0       # a row that has seen nothing
    C[:, Vs:] = 0  # the padding columns are no ids
    Lp = ops.penalize_logits(L, C, RP, PP, FP).to(DEV)  # the reference: fp32 on the CPU
    L = L.to(DEV)
    pos = torch.tensor([3, 9, 5, 11], device=DEV, dtype=torch.int64)
    salt_dev = torch.tensor([123456789], device=DEV, dtype=torch.int64)
    kreq = {}
    if req:
        kreq = dict(row_key=torch.tensor([9, 2, 7, 0], device=DEV, dtype=torch.int64),
                    end=torch.tensor([5, 9, 0, 40], device=DEV, dtype=torch.int64))  # row 1 ends here

    def draw(logits, stop, kw, **pen):
        kw = dict(kw)
        tok = torch.full((B, 1), 777, device=DEV, dtype=torch.int64)
        gen = torch.full((B, G), -5, device=DEV, dtype=torch.int64)
        done = torch.tensor([0, 0, 1, 0], device=DEV, dtype=torch.int64)  # row 2 is finished: skipped
        stats = torch.full((B, 2), -1, device=DEV, dtype=torch.int32) if kw.pop("stats", False) else None
        ops.sample_topk_(logits, T, kw.pop("top_k"), 99, pos, tok, gen, salt_dev=salt_dev, stop_token=stop, done=done,
                         stats=stats, **kw, **kreq, **pen)
        return tok, gen, done, stats

    for kw in SETTINGS:
        t0 = draw(Lp, None, kw)[0]
        stop = int(t0[3])  # what row 3 draws: it finishes by the stop token
        want = draw(Lp, stop, kw)
        cnt = C.to(DEV)
        got = draw(L, stop, kw, counts=cnt, **PEN)
        for a, b in zip(got, want):
            assert (a is None and b is None) or torch.equal(a, b), (kw, got, want)
        assert want[2][2:].tolist() == [1, 1] and (not req or int(want[2][1]) == 1), kw  # skipped, stopped, ended
        grown = C.clone()
        for b in (0, 1, 3):
            grown[b, int(want[0][b])] += 1  # the one-hot of each drawn id, and nowhere else
        assert torch.equal(cnt.cpu(), grown), kw


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("S", [1, 37])
def test_token_counts_kernel(kernels, n, S):
    from nanosandbox_amd import ops

    g = torch.Generator().manual_seed(10 * n + S)
    W = 100
    idx = torch.randint(0, 97, (n, S), generator=g).to(DEV)
    lens = [1, S, (S + 1) // 2][:n]
    lengths = torch.tensor(lens, device=DEV, dtype=torch.int64)
    rows = [3, 0, 2][:n]
    for use_rows in (False, True):
        for use_len in (False, True):
            table = torch.full((4, W), -7, device=DEV, dtype=torch.int32)
            r = torch.tensor(rows, device=DEV, dtype=torch.int64) if use_rows else None
            ops.token_counts_(table, idx, lengths if use_len else None, r)
            want = torch.full((4, W), -7, dtype=torch.int32)
            for i in range(n):
                want[rows[i] if use_rows else i] = _hist(idx[i, :lens[i] if use_len else S], W)
            assert torch.equal(table.cpu(), want)  # untouched rows keep the sentinel
            ops.token_counts_(table, idx, lengths if use_len else None, r, accumulate=True)
            for i in range(n):
                want[rows[i] if use_rows else i] += _hist(idx[i, :lens[i] if use_len else S], W)
            assert torch.equal(table.cpu(), want)


def test_decoder_count_table(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    lens = (5, 40, 33, 9)
    prompts = _prompts(lens)
    idx = torch.zeros(4, 40, device=DEV, dtype=torch.int64)
    for b, p in enumerate(prompts):
        idx[b, :p.numel()] = p
    lengths = torch.tensor(lens, device=DEV)
    dec = Decoder(m, 4, per_row=True, penalize=True)
    try:
        logits = dec.prefill(idx, lengths)
        assert torch.equal(dec.cnt.cpu(), torch.stack([_hist(p) for p in prompts]))
        dec.sample_into(logits, 1.0, 1, **PEN)
        dec.run(3, 1.0, 1, None, **PEN)
        stop = int(dec.gen[2, lens[2] + 2])  # row 2's third token: the greedy rerun stops there at the latest
        logits = dec.prefill(idx, lengths)
        dec.sample_into(logits, 1.0, 1, stop, **PEN)
        dec.run(20, 1.0, 1, stop, **PEN)
        pos, done = dec.pos.tolist(), dec.done.tolist()
        assert done[2] == 1 and pos[2] <= lens[2] + 2 and 0 in done  # a row frozen early, and one that ran on
        texts = [dec.gen[b, lens[b]:pos[b] + 1] for b in range(4)]  # a frozen row's last token is at pos
        for b in range(4):
            if not done[b]:
                assert texts[b].numel() == 21
        assert torch.equal(dec.cnt.cpu(), torch.stack([_hist(torch.cat([p, t])) for p, t in zip(prompts, texts)]))
        # admit: the admitted rows' prompts, every other row bit for bit
        before = dec.cnt.clone()
        new = _prompts((7, 40, 1), seed=8)
        nidx = torch.zeros(3, 40, device=DEV, dtype=torch.int64)
        for i, p in enumerate(new):
            nidx[i, :p.numel()] = p
        dec.admit([3, 0, 2], nidx, torch.tensor([7, 40, 1], device=DEV))
        assert torch.equal(dec.cnt[1], before[1])
        assert torch.equal(dec.cnt[[3, 0, 2]].cpu(), torch.stack([_hist(p) for p in new]))
    finally:
        dec.release()
    # a shared prefix: the prefix's histogram with every row's suffix on top; admit puts cnt0 back
    prefix, sfx = _prompts((11,), seed=9)[0], _prompts((3, 1, 8), seed=10)
    sidx = torch.zeros(3, 8, device=DEV, dtype=torch.int64)
    for i, p in enumerate(sfx):
        sidx[i, :p.numel()] = p
    dec = Decoder(m, 3, per_row=True, shared_prompt=True, max_new=32, penalize=True)
    try:
        dec.prefill_shared(prefix)
        assert torch.equal(dec.cnt.cpu(), _hist(prefix).expand(3, -1))
        logits = dec.prefill_suffixes(sidx, torch.tensor([3, 1, 8], device=DEV))
        assert torch.equal(dec.cnt.cpu(), torch.stack([_hist(torch.cat([prefix, p])) for p in sfx]))
        dec.sample_into(logits, 0.8, 50, **PEN)
        dec.run(5, 0.8, 50, **PEN)
        texts = [torch.cat([prefix, p, dec.gen[b, 11 + p.numel():11 + p.numel() + 6]]) for b, p in enumerate(sfx)]
        assert torch.equal(dec.cnt.cpu(), torch.stack([_hist(t) for t in texts]))
        keep = dec.cnt.clone()
        dec.admit([1])
        assert torch.equal(dec.cnt[1].cpu(), _hist(prefix)) and torch.equal(dec.cnt[[0, 2]], keep[[0, 2]])
    finally:
        dec.release()


def _run(dec, idx, n, temperature, top_k, **pen):
    dec.sample_into(dec.prefill(idx), temperature, top_k, **pen)
    dec.run(n - 1, temperature, top_k, **pen)
    T0 = idx.shape[1]
    return dec.gen[:, T0:T0 + n].clone()


@pytest.mark.parametrize("B", [1, 3])
def test_decoder_is_the_manual_loop(kernels, B):
    """Eager penalising decoder == a plain decoder's step() + ``penalize_logits`` on the CPU + the
    plain sampler, token for token (the same kernels see the same bits); the captured graph gives
    the eager tokens; identity parameters give the plain decoder's."""
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    n, T, k = 24, 0.8, 50
    idx = torch.stack(_prompts((12,) * B, seed=4))
    decs = [Decoder(m, B, use_graph=False), Decoder(m, B, use_graph=False, penalize=True),
            Decoder(m, B, use_graph=True, penalize=True)]
    plain, eager, graph = decs
    try:
        for d in decs:
            d.salt = 424242
        want_plain = _run(plain, idx, n, T, k)
        assert torch.equal(_run(eager, idx, n, T, k), want_plain)  # the identity, through the penalised entry
        assert torch.equal(_run(graph, idx, n, T, k), want_plain)
        got = _run(eager, idx, n, T, k, **PEN)
        assert torch.equal(_run(graph, idx, n, T, k, **PEN), got)
        assert torch.equal(graph.cnt, eager.cnt)
        # the manual loop
        counts = torch.stack([_hist(r) for r in idx])
        logits = plain.prefill(idx)
        for i in range(n):
            lp = ops.penalize_logits(logits.float().cpu(), counts, RP, PP, FP).to(DEV)
            ops.sample_topk_(lp, T, k, plain.salt, plain.pos, plain.tok, plain.gen, salt_dev=plain.salt_dev)
            counts[torch.arange(B), plain.tok.view(-1).cpu()] += 1
            if i + 1 < n:
                logits = plain.step(plain.tok)
        assert torch.equal(plain.gen[:, 12:12 + n], got)
        assert torch.equal(eager.cnt.cpu(), counts)
        assert not torch.equal(got, want_plain)
    finally:
        for d in decs:
            d.release()


def _no_repeats(outs, prompts, n):
    for o, p in zip(outs, prompts):
        new = o[p.numel():].tolist()
        assert torch.equal(o[:p.numel()], p) and len(new) == n
        assert len(set(new)) == n and not set(new) & set(p.tolist()), (p.tolist(), new)


@pytest.mark.parametrize("mode", ["bf16", "q8", "kv8", "prefix", "queue"])
def test_a_huge_presence_penalty_forbids_repeats(kernels, mode):
    m = _model()
    n = 48
    kw = dict(top_k=1, presence_penalty=1e4)
    if mode == "prefix":
        base = _distinct((30,), seed=3)[0]
        prompts = [torch.cat([base[:8], base[8 + 5 * i:8 + 5 * i + 2 + i]]) for i in range(4)]
        kw.update(shared_prefix=True)
    else:
        prompts = _distinct((5, 40, 33, 9, 17))
        kw.update(dict(q8=dict(quantize="int8"), kv8=dict(kv_quantize="int8"), queue=dict(batch_size=2)).get(mode, {}))
    _no_repeats(m.generate_batch(prompts, n, **kw), prompts, n)
    assert not any(hasattr(p, "compute") for p in m.parameters())


def test_queue_rows_start_from_the_prompts_counts(kernels):
    m = _model()
    p = _prompts((11,), seed=9)[0]
    budgets = [24, 3, 17, 1, 9, 24, 12]
    outs = []
    for bs in (2, 4):
        torch.manual_seed(7)
        outs.append(m.generate_batch([p] * 7, budgets, temperature=0.8, top_k=50, shared_prompt=True, batch_size=bs,
                                     **PEN))
    assert all(torch.equal(a, b) for a, b in zip(*outs))  # no count survives from a row's previous request
    assert all(a.numel() == 11 + k for a, k in zip(outs[0], budgets))
    torch.manual_seed(7)
    off = m.generate_batch([p] * 7, budgets, temperature=0.8, top_k=50, shared_prompt=True, batch_size=2)
    assert not all(torch.equal(a, b) for a, b in zip(outs[0], off))


def test_speculation_with_penalties_is_refused(kernels):
    from nanosandbox_amd.runtime.decode import Decoder

    m = _model()
    with pytest.raises(ValueError):
        Decoder(m, 2, speculate=2, penalize=True)
    with pytest.raises(ValueError):
        m.generate_batch(_prompts((5, 9)), 8, speculate=2, repetition_penalty=1.3)
    with pytest.raises(RuntimeError):  # the C entry point refuses what the Python checks would
        from nanosandbox_amd.ops import _lib
        t = torch.zeros(1, 8, device=DEV)
        c = torch.zeros(1, 8, device=DEV, dtype=torch.int32)
        i64 = torch.zeros(1, 8, device=DEV, dtype=torch.int64)
        _lib.call("nsa_sample_penalized", _lib.ptr(t), 1, 8, 8, 1.0, 0, 0, 1.0, 0.0, 1, None, _lib.ptr(i64), 0,
                  _lib.ptr(i64), _lib.ptr(i64), 8, -1, None, None, None, None, _lib.ptr(c), 8, 0.0, 0.0, 0.0,
                  _lib.stream())
