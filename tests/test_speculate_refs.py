"""Speculative decoding on the CPU: the reference forms of ``ops.ngram_draft`` / ``ops.spec_accept_``
against brute-force loops written from the rule, ``ops.decode_attention_spec`` against successive
single-query calls, and ``Decoder(..., speculate=K)`` against the plain decoder, token for token
(runtime/decode.py).  ``draft_cases`` / ``accept_cases`` are also what the GPU kernel is held to
(tests/test_speculate_gpu.py)."""

import pytest
import torch

I64 = torch.int64


# ---------------------------------------------------------------------------------------------
# drafting

def _brute_draft(h, p, K, N):
    """The rule, as the issue states it: n from N down to 1 (n <= p), the most recent earlier
    occurrence of h[p-n+1 .. p] starting at s with s + n <= p, continued with period L."""
    for n in range(N, 0, -1):
        if n > p:
            continue
        best = None
        for s in range(0, p - n + 1):
            if all(h[s + i] == h[p - n + 1 + i] for i in range(n)):
                best = s
        if best is not None:
            L = p + 1 - (best + n)
            return [h[best + n + (i % L)] for i in range(K)]
    return [h[p]] * K


def draft_cases():
    """name -> (gen [B, T + 1], pos [B], tok [B, 1], K, N, T, table or None)."""
    T = 40
    rows = {
        # 3-gram (7, 8, 9) seen before: continue with what followed it
        "n3": ([1, 7, 8, 9, 4, 5, 6, 2, 7, 8, 9], 10),
        # only the last 2 / the last 1 token(s) seen before: n falls back from 3
        "n2": ([1, 3, 8, 9, 4, 5, 6, 2, 7, 8, 9], 10),
        "n1": ([1, 3, 8, 2, 9, 5, 6, 2, 7, 8, 9], 10),
        "none": ([1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11], 10),
        # the match ends at p - 1: L = 1, one token repeated
        "L1": ([4, 6, 5, 5, 5], 4),
        # a loop of period 3 drafted whole: K > L
        "loop": ([9, 1, 2, 3, 1, 2, 3, 1, 2], 8),
        # the most recent of two occurrences wins
        "recent": ([5, 6, 1, 0, 5, 6, 2, 0, 5, 6], 9),
        "p0": ([3], 0),
        "p1_same": ([3, 3], 1),
    }
    g = torch.Generator().manual_seed(4)
    for i in range(6):  # random histories over a small alphabet: matches at every n
        p = int(torch.randint(1, T, (1,), generator=g))
        rows[f"rand{i}"] = (torch.randint(0, 3 + i, (p + 1,), generator=g).tolist(), p)
    rows["full"] = (torch.randint(0, 4, (T + 1,), generator=g).tolist(), T)  # a finished row at the cache's end
    names = list(rows)
    gen = torch.full((len(names), T + 1), -1, dtype=I64)
    for b, k in enumerate(names):
        h, p = rows[k]
        gen[b, :len(h)] = torch.tensor(h)
    pos = torch.tensor([rows[k][1] for k in names], dtype=I64)
    tok = torch.stack([gen[b, p] for b, p in enumerate(pos.tolist())]).view(-1, 1)
    table = torch.randint(0, 99, (len(names), T + 1), generator=g)
    cases = {}
    for K in (1, 4, 7):
        for N in (1, 3, 5):
            cases[f"ngram K{K} N{N}"] = (gen, pos, tok, K, N, T, None)
        cases[f"table K{K}"] = (gen, pos, tok, K, 3, T, table)
    return cases


@pytest.mark.parametrize("name", list(draft_cases()))
def test_ngram_draft(name):
    from nanosandbox_amd import ops

    gen, pos, tok, K, N, T, table = draft_cases()[name]
    stok, spos, cpos = ops.ngram_draft(gen, pos, tok, K, N, T, table)
    for b, p in enumerate(pos.tolist()):
        if table is None:
            want = _brute_draft(gen[b].tolist(), p, K, N)
        else:
            want = [int(table[b, min(p + 1 + i, T)]) for i in range(K)]
        assert stok[b].tolist() == [int(tok[b])] + want, (name, b)
        assert spos[b].tolist() == [min(p + j, T - 1) for j in range(K + 1)]
        assert cpos[b].tolist() == [min(p + j + 1, T) for j in range(K + 1)]


def test_ngram_draft_named_cases():
    """What the hand-made histories are there for, spelled out."""
    from nanosandbox_amd import ops

    gen, pos, tok, K, N, T, _ = draft_cases()["ngram K4 N3"]
    stok = ops.ngram_draft(gen, pos, tok, K, N, T)[0][:, 1:].tolist()
    assert stok[0] == [4, 5, 6, 2]   # n = 3
    assert stok[1] == [4, 5, 6, 2]   # n = 2
    assert stok[2] == [5, 6, 2, 7]   # n = 1: the 9 at position 4
    assert stok[3] == [11] * 4       # no match
    assert stok[4] == [5] * 4        # L = 1
    assert stok[5] == [3, 1, 2, 3]   # K > L = 3
    assert stok[6] == [2, 0, 5, 6]   # the later occurrence
    assert stok[7] == [3] * 4 and stok[8] == [3] * 4


# ---------------------------------------------------------------------------------------------
# accepting

def _brute_accept(st, b):
    """One row of the accept rule -> (gen row, pos, tok, done, stats row)."""
    K, T, stop = st["cand"].shape[1] - 1, st["T"], st["stop"]
    gen, p, tok, done = st["gen"][b].tolist(), int(st["pos"][b]), int(st["tok"][b]), int(st["done"][b])
    stats = st["stats"][b].tolist()
    if done:
        return gen, p, tok, done, stats
    limit = min(T, int(st["end"][b]))
    cand, draft = st["cand"][b].tolist(), st["stok"][b, 1:].tolist()
    n = 0
    while n < K and draft[n] == cand[n] and p + (n + 1) + 1 <= limit:
        n += 1
    emitted = 0
    for i in range(n + 1):
        gen[p + 1 + i] = cand[i]
        tok = cand[i]
        emitted += 1
        if cand[i] == stop:
            done = 1
            break
    stats = [stats[0] + 1, stats[1] + min(K, limit - p - 1), stats[2] + emitted - 1]
    p += emitted
    if p >= limit:
        done = 1
    return gen, p, tok, done, stats


ACCEPT_T = 32
ACCEPT_ROWS = [  # (name, pos, end, done, draft, cand); the stop token is 7
    ("all right", 10, 99, 0, [11, 12, 13, 14], [11, 12, 13, 14, 15]),
    ("first wrong", 10, 99, 0, [11, 12, 13, 14], [21, 12, 13, 14, 15]),
    ("third wrong", 10, 99, 0, [11, 12, 13, 14], [11, 12, 23, 14, 15]),
    ("stop in the run", 10, 99, 0, [11, 7, 13, 14], [11, 7, 13, 14, 15]),
    ("stop drawn first", 10, 99, 0, [11, 12, 13, 14], [7, 12, 13, 14, 15]),
    ("stop as the bonus token", 10, 99, 0, [11, 12, 13, 14], [11, 12, 13, 14, 7]),
    ("end cuts the run", 10, 13, 0, [11, 12, 13, 14], [11, 12, 13, 14, 15]),
    ("end at the next token", 10, 11, 0, [11, 12, 13, 14], [11, 12, 13, 14, 15]),
    ("T cuts the run", ACCEPT_T - 3, 99, 0, [11, 12, 13, 14], [11, 12, 13, 14, 15]),
    ("last cache row", ACCEPT_T - 1, 99, 0, [11, 12, 13, 14], [11, 12, 13, 14, 15]),
    ("done row", 10, 99, 1, [11, 12, 13, 14], [11, 12, 13, 14, 15]),
]


def accept_cases():
    """name -> the arguments of ``spec_accept_`` as a dict of tensors (and T, N, stop, table), one
    batch row per entry of ``ACCEPT_ROWS``."""
    T, K, rows = ACCEPT_T, 4, ACCEPT_ROWS
    g = torch.Generator().manual_seed(5)
    B = len(rows)
    gen = torch.randint(0, 6, (B, T + 1), generator=g)  # a small alphabet: the next drafts find matches
    st = dict(T=T, N=3, stop=7, table=None,
              gen=gen, pos=torch.tensor([r[1] for r in rows], dtype=I64),
              end=torch.tensor([r[2] for r in rows], dtype=I64), done=torch.tensor([r[3] for r in rows], dtype=I64),
              cand=torch.tensor([r[5] for r in rows], dtype=I64), stats=torch.arange(3 * B, dtype=I64).view(B, 3),
              spos=torch.zeros(B, K + 1, dtype=I64), cpos=torch.zeros(B, K + 1, dtype=I64))
    st["tok"] = torch.stack([gen[b, r[1]] for b, r in enumerate(rows)]).view(B, 1)
    st["stok"] = torch.cat([st["tok"], torch.tensor([r[4] for r in rows], dtype=I64)], dim=1)
    cases = {"ngram": st, "no stop token": dict(st, stop=None)}
    cases["table"] = dict(st, table=torch.randint(0, 99, (B, T + 1), generator=g))
    return cases


@pytest.mark.parametrize("name", ["ngram", "no stop token", "table"])
def test_spec_accept(name):
    from nanosandbox_amd import ops

    case, names = accept_cases()[name], [r[0] for r in ACCEPT_ROWS]
    st = {k: (v.clone() if torch.is_tensor(v) else v) for k, v in case.items()}
    ops.spec_accept_(st["cand"], st["stok"], st["spos"], st["cpos"], st["gen"], st["pos"], st["tok"], st["done"],
                     st["end"], T=st["T"], N=st["N"], stop_token=st["stop"], table=st["table"], stats=st["stats"])
    T, K = st["T"], st["cand"].shape[1] - 1
    for b, row in enumerate(names):
        gen, p, tok, done, stats = _brute_accept(case, b)
        assert st["gen"][b].tolist() == gen, row
        assert (int(st["pos"][b]), int(st["tok"][b]), int(st["done"][b])) == (p, tok, done), row
        assert st["stats"][b].tolist() == stats, row
        # the same launch drafts for the next step, from the new position
        if st["table"] is None:
            want = _brute_draft(gen, p, K, st["N"])
        else:
            want = [int(st["table"][b, min(p + 1 + i, T)]) for i in range(K)]
        assert st["stok"][b].tolist() == [tok] + want, row
        assert st["spos"][b].tolist() == [min(p + j, T - 1) for j in range(K + 1)], row
    if name == "ngram":  # the named outcomes, spelled out: emitted tokens and the finished flag
        moved = (st["pos"] - case["pos"]).tolist()
        assert moved == [5, 1, 3, 2, 1, 5, 3, 1, 3, 1, 0]
        assert st["done"].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1]


# ---------------------------------------------------------------------------------------------
# the attention's reference form

@pytest.mark.parametrize("S", [2, 5])
def test_attention_reference_is_successive_single_queries(S):
    from nanosandbox_amd import ops

    torch.manual_seed(1)
    B, H, D, T = 3, 2, 16, 24
    positions = [0, 9, T - 2]  # the last row: dead queries
    pos = torch.tensor(positions, dtype=I64)
    qkv = torch.randn(B, S, 3 * H * D)
    kc, vc = torch.randn(B, H, T, D), torch.randn(B, H, T, D)
    rk, rv = kc.clone(), vc.clone()
    out = ops.decode_attention_spec(qkv, kc, vc, pos, H)
    for j in range(S):
        for b, p in enumerate(positions):
            if p + j >= T:
                assert bool((out[b, j] == 0).all())
                continue
            one = slice(b, b + 1)
            want = ops.decode_attention(qkv[one, j:j + 1], rk[one], rv[one], pos[one] + j, H, append=True)
            assert torch.equal(out[b, j], want[0, 0])
    assert torch.equal(kc, rk) and torch.equal(vc, rv)
    c = ops.QuantCache(torch.zeros(B, H, T, D, dtype=torch.int8), torch.ones(B, H, T))
    with pytest.raises(AssertionError):
        ops.decode_attention_spec(qkv, c, c, pos, H)


# ---------------------------------------------------------------------------------------------
# the decoder

def _tiny(block=48, V=64, seed=0):
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(seed)
    return GPT(GPTConfig(block_size=block, vocab_size=V, n_layer=2, n_head=2, n_embd=32, dropout=0.0, bias=True)).eval()


@pytest.fixture(scope="module")
def tiny():
    m = _tiny()
    g = torch.Generator().manual_seed(2)
    idx = torch.randint(0, 64, (2, 6), generator=g)
    prompts = [torch.randint(0, 64, (k,), generator=g) for k in (3, 18, 11)]  # 18 + 30 == block_size
    plain_cached = m.generate_cached(idx, 30, top_k=1)
    free = m.generate_batch(prompts, 30, top_k=1)
    new = [f[p.numel():].tolist() for f, p in zip(free, prompts)]
    stop = next(x[k] for x in new for k in range(1, len(x)) if x.index(x[k]) >= 1 and any(x[k] not in y for y in new))
    plain_batch = m.generate_batch(prompts, 30, top_k=1, stop_token=stop)
    return m, idx, prompts, stop, plain_cached, plain_batch


@pytest.mark.parametrize("K", [1, 4, 7])
def test_greedy_equals_the_plain_decoder(tiny, K):
    m, idx, prompts, stop, plain_cached, plain_batch = tiny
    assert torch.equal(m.generate_cached(idx, 30, top_k=1, speculate=K), plain_cached)
    out = m.generate_batch(prompts, 30, top_k=1, stop_token=stop, speculate=K)
    assert len(out) == len(plain_batch) and all(torch.equal(a, b) for a, b in zip(out, plain_batch))
    assert any(a.numel() < p.numel() + 30 for a, p in zip(out, prompts))  # the stop token cut a row
    assert prompts[1].numel() + 30 == m.config.block_size
    assert not any(hasattr(p, "compute") for p in m.parameters())


def test_ngram_acceptance_count():
    """The queue test's tiny model cycles within a few tokens under greedy decoding, and the
    n-gram drafter (K = 4, N = 3) then needs 24-25 steps for 120 new tokens: at most half the
    plain decoder's steps is asserted, and the counters' identity."""
    from nanosandbox_amd.models import GPT, GPTConfig
    from nanosandbox_amd.runtime.decode import batch_decoder

    torch.manual_seed(0)
    m = GPT(GPTConfig(block_size=256, vocab_size=512, n_layer=3, n_head=4, n_embd=256, dropout=0.0, bias=False)).eval()
    g = torch.Generator().manual_seed(6)
    prompts = [torch.randint(0, 512, (k,), generator=g) for k in (5, 40, 33)]
    N = 120
    dec = batch_decoder(m, prompts, N, speculate=4, spec_ngram=3)
    try:
        out = m.generate_batch(prompts, N, top_k=1, speculate=4, spec_ngram=3, decoder=dec)
        st = dec.spec_stats
        assert dec.fits(3, per_row=True, speculate=4, spec_ngram=3) and not dec.fits(3, per_row=True)
        assert not dec.fits(3, per_row=True, speculate=4, spec_ngram=2) and not dec.fits(3, True, speculate=5)
    finally:
        dec.release()
    print("live steps", st["steps"], "accepted", st["accepted"], "offered", st["offered"])
    assert all(a.numel() == p.numel() + N for a, p in zip(out, prompts))
    for b in range(3):
        assert st["steps"][b] <= N // 2
        assert st["accepted"][b] + st["steps"][b] == N - 1
        assert st["accepted"][b] <= st["offered"][b] <= 4 * st["steps"][b]


def test_refusals():
    from nanosandbox_amd.runtime.decode import Decoder

    m = _tiny()
    idx = torch.zeros(2, 4, dtype=I64)
    prompts = [torch.zeros(4, dtype=I64), torch.zeros(4, dtype=I64)]
    for kw in (dict(kv_quantize="int8"), dict(shared_prompt=True)):
        with pytest.raises(ValueError):
            m.generate_cached(idx, 8, speculate=2, **kw)
        with pytest.raises(ValueError):
            m.generate_batch(prompts, 8, speculate=2, **kw)
        with pytest.raises(ValueError):
            Decoder(m, 2, speculate=2, **dict(kw, max_new=8) if "shared_prompt" in kw else kw)
    with pytest.raises(ValueError):
        m.generate_batch(prompts, 8, speculate=2, shared_prefix=True)
    for kw in (dict(batch_size=1), dict(batch_size=2)):
        with pytest.raises(ValueError):
            m.generate_batch(prompts, 8, speculate=2, **kw)
    with pytest.raises(ValueError):
        m.generate_batch(prompts, [8, 4], speculate=2)
    for bad in (8, -1):
        with pytest.raises(ValueError):
            m.generate_cached(idx, 8, speculate=bad)
    with pytest.raises(ValueError):
        m.generate_cached(idx, 8, speculate=2, spec_ngram=0)
    with pytest.raises(ValueError):  # no recompute loop under speculation
        m.generate_cached(idx, m.config.block_size, speculate=2)
    dec = Decoder(m, 2, speculate=2)
    try:
        assert dec.per_row and dec.K == 2 and dec.N == 3
        with pytest.raises(ValueError):
            dec.serve(prompts, [4, 4])
        with pytest.raises(ValueError):
            dec.run(2, queue=True)
    finally:
        dec.release()
    # speculate 0 / None: the plain decoder, nothing speculative about it
    for off in (0, None):
        dec = Decoder(m, 2, speculate=off)
        assert dec.K == 0 and not dec.per_row and dec.fits(2)
        dec.release()
