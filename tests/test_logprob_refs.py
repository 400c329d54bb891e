"""Log-probabilities of drawn and given tokens, on the CPU: the torch rule of ``ops.token_logprobs``
against a float64 brute force, an fp32 emulation of the kernel's own summation order against float64
(which sets the constant of the GPU bound), ``GPT.score`` against cross-entropy, and the front ends.

The bound of the GPU tests.  u = 2^-24 is the relative rounding error of one fp32 operation.  The
kernel forms lp = (l[id] - m) - log(S), S = sum_j exp(l[j] - m), with m exact (a maximum) and the
inputs exact (bf16 widens exactly).  With a_j = m - l[j] >= 0 and p_j = exp(-a_j) / S, to first order:

* ``l[j] - m`` is rounded once: the exponent moves by at most u a_j, term j by the factor u a_j, and S
  by the relative amount u sum_j p_j a_j = u (H - ln S) <= u ln V (H <= ln V the entropy, S >= 1);
* exp is within 1 ulp <= 2 u of every term, so of S;
* every addition on the way to S adds at most u to the relative error of a partial sum of
  non-negative terms, and the deepest path has D(V) of them: the serial adds of one accumulator
  (column i goes to accumulator i % (8 NT): ceil(V / (8 NT)) of them, counting the first onto 0), 3 to
  fold a thread's 8 accumulators, 6 for the butterfly over 64 lanes and log2(NT / 64) for the one over
  the wave sums, where NT = 256 for V <= 14336, 1024 for V <= 57344 and 256 beyond;
* a relative error e of S is an absolute error e of log S, and log is within 1 ulp <= 2 u of its
  result ln S <= ln V;
* ``l[id] - m`` and the last subtraction are rounded once each: at most u a_id + u |lp| <= 2 u |lp|.

Together u (D(V) + 2 + 3 ln V + 2 |lp|).  The part that does not scale with |lp| is doubled, for the
second-order terms and for a library exp or log that is good to 2 ulp rather than 1:

    |lp_kernel - lp_float64| <= 2^-24 (c(V) + 2 |lp|),   c(V) = 2 (D(V) + 2 + 3 ln V).

At V = 50304: D = 7 + 3 + 6 + 4 = 20, c = 109.0, 6.5e-6 + 1.2e-7 |lp|.  The alternatives' log-probabilities
are formed by the same expression and obey the same bound with their own |lp|.  Nothing here was
tuned on a GPU.  The torch rule sums in an order of torch's choosing, so its test uses the bound of
any order, D = V - 1."""

import math

import pytest
import torch

F64 = torch.float64
U = 2.0 ** -24
NEG = -float("Inf")


def kernel_threads(V):
    return 256 if V <= 14336 else 1024 if V <= 57344 else 256


def depth(V):
    NT = kernel_threads(V)
    return -(-V // (8 * NT)) + 3 + 6 + int(math.log2(NT // 64))


def bound(V, lp, D=None):
    """2^-24 (c(V) + 2 |lp|) elementwise (``lp``: float64 reference values; -inf stays exact: 0)."""
    c = 2.0 * ((depth(V) if D is None else D) + 2.0 + 3.0 * math.log(V))
    a = torch.where(torch.isinf(lp), torch.zeros_like(lp), lp.abs())
    return U * (c + 2.0 * a)


def within(got, want, V, D=None):
    """Elementwise: fp32 ``got`` within the bound of float64 ``want``; an infinite value must be met exactly."""
    got, want = got.to(F64).cpu(), want.to(F64)
    exact = torch.isinf(want) | torch.isinf(got)
    err = torch.where(exact, (got != want).to(F64), (got - want).abs())  # NaN fails every comparison
    return err <= bound(V, want, D)


def adversarial_rows(V, M, seed=0, scale=3.0):
    """fp32 [M, V]: the row kinds cycle through flat, a +80 spike, -inf columns, signed-zero ties,
    duplicates of the maximum and plain normal rows."""
    g = torch.Generator().manual_seed(1000 * seed + V)
    L = torch.randn(M, V, generator=g) * scale
    for r in range(M):
        kind = r % 6
        if kind == 0:
            L[r] = 1.25  # flat: sum = V exactly
        elif kind == 1:
            L[r, int(torch.randint(0, V, (1,), generator=g))] += 80.0
        elif kind == 2 and V > 1:
            L[r, torch.rand(V, generator=g) < 0.5] = NEG
            L[r, int(torch.randint(0, V, (1,), generator=g))] = 0.5  # the maximum stays finite
        elif kind == 3:
            z = torch.where(torch.rand(V, generator=g) < 0.5, torch.tensor(0.0), torch.tensor(-0.0))
            L[r] = torch.where(torch.rand(V, generator=g) < 0.7, z, -L[r].abs())
        elif kind == 4:
            L[r, torch.rand(V, generator=g) < 0.1] = 9.0
            L[r, V // 2] = 9.0
    return L


def brute(L, ids, N):
    """float64: (lp [M], top_ids [M, N], top_lp [M, N]) for in-range ids; order (logit desc, id asc)."""
    M, V = L.shape
    l = L.to(F64)
    m = l.max(dim=-1, keepdim=True).values
    lse = m + torch.log(torch.exp(l - m).sum(-1, keepdim=True))
    lp = (l.gather(1, ids.clamp(0, V - 1).view(M, 1)) - lse).view(M)
    top_ids = torch.full((M, N), -1, dtype=torch.int32)
    top_lp = torch.full((M, N), NEG, dtype=F64)
    if N:
        # a stable descending sort of float values: -0.0 == 0.0, the lower id first
        ls, order = torch.sort(l + 0.0, dim=-1, descending=True, stable=True)
        n = min(N, V)
        top_ids[:, :n] = order[:, :n].to(torch.int32)
        top_lp[:, :n] = ls[:, :n] - lse
    return lp, top_ids, top_lp


def emulate_kernel_lse(row):
    """log S of one fp32 row in the kernel's order, every operation in fp32."""
    V = row.numel()
    NT = kernel_threads(V)
    m = row.max()
    w = torch.exp(row - m)  # fp32
    J = -(-V // (8 * NT))
    pad = torch.zeros(J * NT * 8)
    pad[:V] = w
    acc = torch.zeros(NT, 8)
    for part in pad.view(J, NT, 8):
        acc = acc + part  # column i onto accumulator (i / 8 % NT, i % 8), in ascending i
    v = ((acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])) + ((acc[:, 4] + acc[:, 5]) + (acc[:, 6] + acc[:, 7]))
    v = v.view(NT // 64, 64)
    lane = torch.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ off]
    r = v[:, 0]
    w_ = torch.arange(NT // 64)
    off = NT // 128
    while off:
        r = r + r[w_ ^ off]
        off //= 2
    assert bool((r == r[0]).all())  # every wave ends with the same bits
    return m, torch.log(r[0])


@pytest.mark.parametrize("V", [1, 2, 5, 63, 64, 65, 1025])
def test_torch_rule_matches_float64(V):
    from nanosandbox_amd import ops

    M, N = 13, 8
    L = adversarial_rows(V, M)
    g = torch.Generator().manual_seed(V)
    ids = torch.randint(0, V, (M,), generator=g)
    ids[5], ids[7] = -1, V  # skipped rows
    out = ops.LogProbs(torch.full((M,), float("nan")), torch.full((M, N), -7, dtype=torch.int32),
                       torch.full((M, N), float("nan")))
    got = ops.token_logprobs(L, ids, top=N, out=out)
    lp, top_ids, top_lp = brute(L, ids, N)
    for r in range(M):
        if r in (5, 7):  # nothing written
            assert math.isnan(float(got.token[r])) and bool((got.top_ids[r] == -7).all())
            assert bool(torch.isnan(got.top[r]).all())
            continue
        assert bool(within(got.token[r], lp[r], V, D=V - 1)), (V, r)
        assert torch.equal(got.top_ids[r], top_ids[r]), (V, r)  # exactly the stable sort's
        assert bool(within(got.top[r], top_lp[r], V, D=V - 1).all()), (V, r)
    if V < N:  # slots past V: id -1 and -inf
        assert bool((got.top_ids[0, V:] == -1).all()) and bool((got.top[0, V:] == NEG).all())
    flat = float(got.token[0])
    assert abs(flat + math.log(V)) <= float(bound(V, torch.tensor(-math.log(V), dtype=F64), D=V - 1))
    # without ``out``: fresh buffers, NaN / -1 in the skipped rows
    fresh = ops.token_logprobs(L, ids, top=2)
    assert math.isnan(float(fresh.token[5])) and fresh.top_ids[7].tolist() == [-1, -1]
    assert torch.equal(fresh.token[:5], got.token[:5])
    # bf16 input and a V smaller than the row: the padding columns are no ids
    if V > 2:
        Lb = L.to(torch.bfloat16)
        a = ops.token_logprobs(Lb, ids.clamp(0, V - 2), top=1, V=V - 1)
        b = ops.token_logprobs(Lb.float()[:, :V - 1].contiguous(), ids.clamp(0, V - 2), top=1)
        assert torch.equal(a.token, b.token) and torch.equal(a.top_ids, b.top_ids)


@pytest.mark.parametrize("V", [1, 7, 65, 2049, 14336, 14337, 50257, 50304, 57345])
def test_kernel_order_in_fp32_stays_within_the_bound(V):
    L = adversarial_rows(V, 6, seed=1)
    g = torch.Generator().manual_seed(V)
    ids = torch.randint(0, V, (6,), generator=g)
    lp64, _, _ = brute(L, ids, 0)
    worst = 0.0
    for r in range(6):
        m, logz = emulate_kernel_lse(L[r])
        lp = (L[r, ids[r]] - m) - logz  # fp32, as the kernel forms it
        if math.isinf(float(lp64[r])):
            assert float(lp) == float(lp64[r])
            continue
        err, b = abs(float(lp) - float(lp64[r])), float(bound(V, lp64[r]))
        worst = max(worst, err / b)
        assert err <= b, (V, r, err, b)
    print(f"V={V}: worst error / bound = {worst:.3f}")
    if V == 50304:  # plausibility: below 1e-5 for a log-probability of ordinary size
        assert float(bound(V, torch.tensor(-20.0, dtype=F64))) < 1e-5 and depth(V) == 20


def _tiny(block_size=32, vocab=65):
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(3)
    return GPT(GPTConfig(block_size=block_size, vocab_size=vocab, n_layer=2, n_head=2, n_embd=32, dropout=0.0,
                         bias=True)).eval()


def test_score_is_minus_cross_entropy():
    import torch.nn.functional as F

    m = _tiny()
    g = torch.Generator().manual_seed(0)
    idx = torch.randint(0, 65, (3, 17), generator=g)
    s = m.score(idx, top=3)
    logits = m.forward_logits(idx)[:, :-1]
    want = -F.cross_entropy(logits.reshape(-1, 65), idx[:, 1:].reshape(-1), reduction="none").view(3, 16)
    torch.testing.assert_close(s.token, want, atol=1e-4, rtol=1e-4)
    assert torch.equal(s.top_ids[..., 0].long(), logits.argmax(-1))
    assert s.top_ids.shape == (3, 16, 3) and s.top.shape == (3, 16, 3)
    # lengths: entries at or past a row's last given token are skipped
    lens = torch.tensor([17, 9, 2])
    t = m.score(idx, lengths=lens, top=1)
    for b, n in enumerate(lens.tolist()):
        assert torch.equal(t.token[b, :n - 1], s.token[b, :n - 1])
        assert bool(torch.isnan(t.token[b, n - 1:]).all()) and bool((t.top_ids[b, n - 1:] == -1).all())
    ppl = t.perplexity()
    for b, n in enumerate(lens.tolist()):
        assert abs(float(ppl[b]) - math.exp(-float(s.token[b, :n - 1].mean()))) < 1e-3


def test_generate_cached_logprobs_equal_score_of_the_text():
    m = _tiny()
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, 65, (2, 5), generator=g)
    torch.manual_seed(7)
    y, lp = m.generate_cached(idx, 9, temperature=0.9, top_k=20, logprobs=2)
    torch.manual_seed(7)
    y0 = m.generate_cached(idx, 9, temperature=0.9, top_k=20)
    assert torch.equal(y, y0)  # the same ids as without the keyword
    assert lp.token.shape == (2, 9) and lp.top_ids.shape == (2, 9, 2) and lp.top.shape == (2, 9, 2)
    s = m.score(y, top=2)
    torch.testing.assert_close(lp.token, s.token[:, 4:], atol=1e-4, rtol=1e-4)
    assert torch.equal(lp.top_ids, s.top_ids[:, 4:])
    # penalties change the draws, not what is recorded: still the raw distribution
    torch.manual_seed(7)
    y, lp = m.generate_cached(idx, 9, top_k=20, repetition_penalty=1.5, presence_penalty=0.3, logprobs=0)
    torch.testing.assert_close(lp.token, m.score(y).token[:, 4:], atol=1e-4, rtol=1e-4)
    # past block_size the recompute loop fills it through the same op
    torch.manual_seed(7)
    y, lp = m.generate_cached(idx, 30, top_k=20, logprobs=1)
    assert y.shape == (2, 35) and lp.token.shape == (2, 30) and bool(torch.isfinite(lp.token).all())
    torch.testing.assert_close(lp.token[:, :20], m.score(y[:, :25]).token[:, 4:], atol=1e-4, rtol=1e-4)
    y, lp = m.generate(idx, 3, logprobs=1)
    torch.testing.assert_close(lp.token, m.score(y).token[:, 4:], atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("queue", [False, True])
def test_generate_batch_logprobs_with_a_stop_token(queue):
    m = _tiny()
    g = torch.Generator().manual_seed(2)
    prompts = [torch.randint(0, 65, (n,), generator=g) for n in (4, 7, 3, 5)]
    kw = dict(temperature=1.0, top_k=30, batch_size=2) if queue else dict(temperature=1.0, top_k=30)
    torch.manual_seed(11)
    plain = m.generate_batch(prompts, 12, **kw)
    stop = int(plain[1][prompts[1].numel() + 3])  # what row 1 draws as its 4th token
    torch.manual_seed(11)
    want = m.generate_batch(prompts, 12, stop_token=stop, **kw)
    torch.manual_seed(11)
    outs, recs = m.generate_batch(prompts, 12, stop_token=stop, logprobs=2, **kw)
    assert len(outs[1]) <= prompts[1].numel() + 4
    for p, o, w, r in zip(prompts, outs, want, recs):
        assert torch.equal(o, w)  # the ids of the call without logprobs, under the same seed
        n = o.numel() - p.numel()
        assert r.token.shape == (n,) and r.top_ids.shape == (n, 2) and r.top.shape == (n, 2)
        assert bool(torch.isfinite(r.token).all())  # the stop token's own entry included
        torch.testing.assert_close(r.token, m.score(o[None]).token[0, p.numel() - 1:], atol=1e-4, rtol=1e-4)
    assert int(outs[1][-1]) == stop


def test_refusals():
    from nanosandbox_amd import ops
    from nanosandbox_amd.runtime.decode import Decoder

    m = _tiny()
    idx = torch.zeros(1, 4, dtype=torch.int64)
    for bad in (9, -1, 1.5, True):
        with pytest.raises(ValueError):
            Decoder(m, 1, logprobs=bad)
        with pytest.raises(ValueError):
            m.generate_cached(idx, 3, logprobs=bad)
        with pytest.raises(ValueError):
            m.generate_batch([idx[0]], 3, logprobs=bad)
        with pytest.raises(ValueError):
            ops.token_logprobs(torch.zeros(1, 4), torch.zeros(1, dtype=torch.int64), top=bad)
        with pytest.raises(ValueError):
            m.score(idx, top=bad)
    with pytest.raises(ValueError, match="speculate"):
        Decoder(m, 1, speculate=2, logprobs=1)
    with pytest.raises(ValueError, match="speculate"):
        m.generate_cached(idx, 3, speculate=2, logprobs=0)
    with pytest.raises(ValueError, match="speculate"):
        m.generate_batch([idx[0]], 3, speculate=2, logprobs=0)
    # a decoder without the buffers is not borrowed for a call that needs them, nor the other way round
    plain, rec = Decoder(m, 1), Decoder(m, 1, logprobs=2)
    assert plain.fits(1) and not plain.fits(1, logprobs=2) and not plain.fits(1, logprobs=0)
    assert rec.fits(1, logprobs=2) and not rec.fits(1) and not rec.fits(1, logprobs=3)
    assert plain.lp is None and rec.lp.shape == (1, 33) and rec.top_ids.shape == (1, 33, 2)


def test_sample_cli_logprobs_and_score(tmp_path, monkeypatch, capsys):
    from nanosandbox_amd import sample

    m = _tiny(block_size=48, vocab=97)
    ck = {"model": m.state_dict(), "model_args": dict(block_size=48, vocab_size=97, n_layer=2, n_head=2, n_embd=32,
                                                      bias=True, dropout=0.0),
          "iter_num": 0, "best_val_loss": 0.0, "config": {}}
    torch.save(ck, tmp_path / "ckpt.pt")
    (tmp_path / "prompts.txt").write_text("1,2,3\n4,5,6,7,8\n")
    (tmp_path / "prompt.txt").write_text("1,2,3")
    start = f"--start=FILE:{tmp_path / 'prompt.txt'}"
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    base = [f"--out_dir={tmp_path}", "--device=cpu", "--max_new_tokens=5", "--top_k=1"]
    # every generation path prints the same greedy sample with the same summed log-probability
    want = None
    for extra in ([start, "--num_samples=1"], [start, "--num_samples=1", "--kv_cache=False"],
                  [start, "--num_samples=2", "--sample_batch=2"], [start, "--num_samples=2", "--serve_batch=2"]):
        plain = sample.main(base + extra)
        capsys.readouterr()
        outs = sample.main(base + extra + ["--logprobs=2"])
        lines = capsys.readouterr().out.splitlines()
        assert outs == plain  # the samples of the run without the key
        heads = [ln for ln in lines if ln.startswith("logprob ")]
        assert len(heads) == len(outs) and all("over 5 tokens, perplexity" in h for h in heads)
        assert sum(ln.startswith("  '") and " | " in ln for ln in lines) == 5 * len(outs)
        total = float(heads[0].split()[1])
        new = [int(t) for t in outs[0].split(",")]
        ref = float(m.score(torch.tensor([new])).token[0, 2:].double().sum())
        assert abs(total - ref) < 1e-3
        want = total if want is None else want
        assert abs(total - want) < 1e-3
    # --score: nothing is generated, every line is scored
    outs = sample.main(base + [f"--prompts_file={tmp_path / 'prompts.txt'}", "--score=True"])
    assert [n for _, n, _ in outs] == [2, 4]
    ref = m.score(torch.tensor([[4, 5, 6, 7, 8]])).token[0].double()
    assert abs(outs[1][0] - float(ref.sum())) < 1e-3 and abs(outs[1][2] - math.exp(-float(ref.mean()))) < 1e-3
    with pytest.raises(ValueError):
        sample.main(base + ["--score=True"])
    with pytest.raises(ValueError):
        sample.main(base + ["--logprobs=9"])
    with pytest.raises(ValueError, match="speculate"):
        sample.main(base + ["--logprobs=1", "--speculate=2"])
