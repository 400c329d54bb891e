"""Generation throughput: nanoGPT's recompute loop vs KV-cache decoding (eager / HIP graph).

Random-init GPT-2 weights of the named size, bf16, a random prompt of --prompt tokens,
--new tokens sampled per sequence (temperature 0.8, top-k 200 as in sample.py; --top_k,
--top_p and --min_p choose other settings, e.g. ``--top_k 0 --top_p 0.9``).  Prints
one JSON line per (model, batch, mode) with new tokens/s over the whole batch and the
per-token latency.

    python scripts/decode_bench.py [--models gpt2,gpt2-xl] [--batches 1,8,64] [--prompt 128] [--new 256]

Per-row positions (``Decoder(per_row=True)``): mode ``rows`` is the graph mode with one
position per sequence at equal prompt lengths (what the per-row step costs beside
``graph``); ``--ragged`` adds mode ``ragged``, the same with unequal prompt lengths
(--prompt/2 .. --prompt spread evenly over the batch, no stop token).  ``--repeat N`` runs
the whole mode list N times, interleaved, for the run-to-run spread.  ``--samples N``
times sample.py's flow for N samples of one prompt: a reused batch-1 decoder N times over
(``sample_loop``) against one ``generate_batch`` of N rows (``sample_batch``).
``--quantize int8`` adds ``graph_int8`` / ``rows_int8``, the ``graph`` / ``rows`` modes on a
``Decoder(quantize="int8")``, next to their bf16 twins in the interleaved mode list.
``--kv_quantize int8`` adds ``graph_kv8`` / ``rows_kv8`` (int8 KV caches,
``Decoder(kv_quantize="int8")``) and, with ``--quantize int8``, ``graph_int8_kv8`` /
``rows_int8_kv8``, each next to its twin; ``--prompt`` sets the context length the steps start
from; a cached run feeds positions prompt .. prompt + new, which must stay below block_size
(``--prompt 896 --new 127`` ends at position 1023).  ``--memory`` adds the decoder's peak
allocated bytes (``torch.cuda.max_memory_allocated`` over construction, prefill and the timed
steps, minus what was allocated before) to each line.
``--shared_prompt`` adds ``rows_shared`` (and ``rows_int8_shared``) after ``rows``: the same
settings on a ``Decoder(shared_prompt=True, max_new=--new + 1)``, every row continuing row 0's
prompt; with it the ``rows`` lines and their shared twins also carry ``ttft_ms``, the time from
the start of the prefill to the first drawn token, and ``--samples`` adds
``sample_batch_shared``.
``--shared_prefix --suffix N`` replaces the mode list by ``prefix_rows`` and ``prefix_shared``
(interleaved, ``--repeat`` times): B prompts made of one random prefix of ``--prompt`` tokens and
unequal random suffixes of 1 .. N tokens, on the unshared per-row decoder (right-padded
``prefill(idx, lengths)``) and on the shared-prefix one (``prefill_shared`` +
``prefill_suffixes``, ``max_new = N + --new + 1``); both lines carry ``ttft_ms``, and the shared
one ``ttft_cached_ms``: the same with the prefix already in the decoder, as in every later round.
``--queue R --budgets LO:HI`` replaces the mode list by ``queue_chunks`` and ``queue_serve``
(interleaved, ``--repeat`` times; with ``--shared_prompt``: ``queue_chunks_shared`` and
``queue_serve_shared``, every request the same prompt): R requests of ``--prompt`` tokens whose
budgets are uniform in LO .. HI from a fixed seed, served on reused, warmed decoders of B rows,
first the way a caller had to (chunks of B through ``generate_batch``, each running to its longest
budget), then as one queue (``generate_batch(batch_size=B)``: ``Decoder.serve``).  Each line holds
the useful tokens/s (sum of budgets / wall time), the steps, the admissions, the share of the
stream's time between the start of an ``admit`` and the end of the first-token draw that follows
it (device events, no extra syncs), and the calibration GEMM.
``--speculate K[,K ...]`` adds ``rows_specK`` after ``rows`` (and ``rows_int8_specK`` after
``rows_int8``): the same settings on a ``Decoder(speculate=K)`` with n-gram drafts (``--spec_ngram``).
``--spec_table right|wrong`` (comma-separated for both) adds ``rows_specK_right`` / ``_wrong``: drafts
read from a table holding the tokens the run will draw (every draft accepted: the ceiling) or those
tokens + 1 (none accepted: the cost of the wider step, the floor); the table comes from an untimed
pass with the same sampling stream.  These lines carry the live ``steps`` per row, the drafts
``accepted`` / ``offered`` and their ratio.
``--penalties RP,PP,FP`` adds ``graph_pen`` / ``rows_pen`` right after ``graph`` / ``rows``: the same
settings on a ``Decoder(penalize=True)`` sampling with that repetition, presence and frequency
penalty (the penalised sampler and its count table beside the plain step of the same run).
``--logprobs N[,N ...]`` adds ``graph_lpN`` / ``rows_lpN`` right after ``graph`` / ``rows``: the same settings on
a ``Decoder(logprobs=N)``, whose step records every drawn token's log-probability and N alternatives
(one more launch per step beside the plain step of the same run).
"""

import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nanosandbox_amd.models import GPT, GPTConfig  # noqa: E402
from nanosandbox_amd.runtime.decode import Decoder  # noqa: E402

SMP = dict(top_k=200, top_p=None, min_p=None)  # the sampling settings of every mode (--top_k / --top_p / --min_p)
PEN = {}  # --penalties: the three penalty keywords of the _pen modes
DIMS = {"gpt2": (12, 12, 768), "gpt2-medium": (24, 16, 1024), "gpt2-large": (36, 20, 1280), "gpt2-xl": (48, 25, 1600)}


def run_cached(model, idx, new, use_graph, quantize=None, kv_quantize=None, pen=False, lp=None):
    B = idx.shape[0]
    dec = Decoder(model, B, use_graph=use_graph, quantize=quantize, kv_quantize=kv_quantize, penalize=pen,
                  logprobs=lp)
    smp = dict(SMP, **PEN) if pen else SMP
    dec.sample_into(dec.prefill(idx), 0.8, **smp)
    if use_graph:
        dec.run(1, 0.8, **smp)  # capture outside the timed loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if use_graph:
        dec.run(new, 0.8, **smp)  # step + sampling + feedback: one graph replay per token
    else:
        for _ in range(new):  # eager step + the same device sampling kernel
            dec.sample_into(dec.step(dec.tok), 0.8, **smp)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec.release()
    return dt


def ragged_lengths(B, prompt):
    """--prompt/2 .. --prompt, spread evenly over the batch."""
    lo = max(1, prompt // 2)
    return [prompt if B == 1 else lo + (prompt - lo) * b // (B - 1) for b in range(B)]


def run_rows(model, idx, new, lengths=None, quantize=None, kv_quantize=None, shared=False, pen=False, lp=None):
    """The graph mode on a per_row decoder: equal lengths, or (lengths) a ragged batch; shared:
    a shared_prompt decoder, every row continuing idx[0].  Returns (seconds of the timed steps,
    seconds from the start of the prefill to the first drawn token).  pen: a penalising decoder,
    sampling with --penalties.  lp: a decoder that records log-probabilities and lp alternatives."""
    B = idx.shape[0]
    if shared:  # slots for the capture step and the timed ones
        dec = Decoder(model, B, use_graph=True, per_row=True, quantize=quantize, shared_prompt=True, max_new=new + 1,
                      penalize=pen, logprobs=lp)
    else:
        dec = Decoder(model, B, use_graph=True, per_row=True, quantize=quantize, kv_quantize=kv_quantize,
                      penalize=pen, logprobs=lp)
    smp = dict(SMP, **PEN) if pen else SMP
    lens = None if lengths is None else torch.tensor(lengths, device=idx.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec.sample_into(dec.prefill_shared(idx[0]) if shared else dec.prefill(idx, lens), 0.8, **smp)
    torch.cuda.synchronize()
    ttft = time.perf_counter() - t0
    dec.run(1, 0.8, **smp)  # capture outside the timed loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec.run(new, 0.8, **smp)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec.release()
    return dt, ttft


def run_spec(model, idx, new, K, ngram, table=None, quantize=None):
    """The graph mode on a speculative decoder.  table: None (n-gram drafts), "right" or "wrong".
    Returns (seconds of the timed steps, the decoder's spec_stats for them)."""
    B = idx.shape[0]
    dec = Decoder(model, B, use_graph=True, speculate=K, spec_ngram=ngram, quantize=quantize)

    def go(n):  # the sampling stream is the decoder's, the same in every pass
        dec.sample_into(dec.prefill(idx), 0.8, **SMP)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dec.run(n, 0.8, **SMP)
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    go(4)  # capture outside the timed loop
    if table:
        go(new)
        y = dec.gen.clone()  # what the timed pass will draw, by position
        dec.set_draft_table(y if table == "right" else (y + 1) % model.config.vocab_size)
        go(4)
    dt = go(new)
    stats = dec.spec_stats
    dec.release()
    return dt, stats


def suffix_lengths(B, n):
    """1 .. n, spread evenly over the batch."""
    return [n if B == 1 else 1 + (n - 1) * b // (B - 1) for b in range(B)]


def run_prefix(model, prefix, suf, lengths, new, shared):
    """Prompts prefix + suf[b, :lengths[b]] on the unshared per-row decoder or (shared) on the
    shared-prefix one; the graph mode.  Returns (seconds of the timed steps, seconds from the
    start of the prefill to the first drawn token: the prefix is encoded inside that window,
    and (shared) the same for a second round, whose prefix the decoder already holds)."""
    B, S = suf.shape
    P = prefix.numel()
    lens = torch.tensor(lengths, device=suf.device)
    if shared:  # slots for the suffixes, the capture step and the timed ones
        dec = Decoder(model, B, use_graph=True, per_row=True, shared_prompt=True, max_new=S + new + 1)
    else:
        dec = Decoder(model, B, use_graph=True, per_row=True)
        idx = torch.cat([prefix[None].expand(B, -1), suf], dim=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if shared:
        dec.prefill_shared(prefix)
        logits = dec.prefill_suffixes(suf, lens)
    else:
        logits = dec.prefill(idx, lens + P)
    dec.sample_into(logits, 0.8, **SMP)
    torch.cuda.synchronize()
    ttft = time.perf_counter() - t0
    dec.run(1, 0.8, **SMP)  # capture outside the timed loop
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    dec.run(new, 0.8, **SMP)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    cached = None
    if shared:
        t0 = time.perf_counter()
        dec.prefill_shared(prefix)
        dec.sample_into(dec.prefill_suffixes(suf, lens), 0.8, **SMP)
        torch.cuda.synchronize()
        cached = time.perf_counter() - t0
    dec.release()
    return dt, ttft, cached


def run_samples(model, prompt, n, new, batched, shared=False):
    """sample.py's flow for n samples of one prompt, decoder construction and capture
    included: one batch-1 decoder reused n times, or one generate_batch of n rows (shared: on
    a shared_prompt decoder)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if batched:
        dec = (Decoder(model, n, max_len=model.config.block_size, per_row=True, shared_prompt=True, max_new=new)
               if shared else Decoder(model, n, max_len=model.config.block_size, per_row=True))
        model.generate_batch([prompt] * n, new, temperature=0.8, **SMP, decoder=dec, shared_prompt=shared)
    else:
        dec = Decoder(model, 1, max_len=model.config.block_size)
        for _ in range(n):
            model.generate_cached(prompt[None], new, temperature=0.8, **SMP, decoder=dec)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    dec.release()
    return dt


def queue_budgets(R, lo, hi):
    """R budgets uniform in lo .. hi, from a fixed seed."""
    g = torch.Generator().manual_seed(1234)
    return torch.randint(lo, hi + 1, (R,), generator=g).tolist()


def run_queue(model, prompts, budgets, B, serve, shared):
    """The requests in chunks of B, each to its longest budget, or (serve) as one queue through B
    rows, on a decoder built and warmed (graphs captured) outside the timed window.  Returns
    (seconds, steps, admissions, seconds between the start of an admission and the end of its
    first-token draw)."""
    need = max(budgets)
    dec = (Decoder(model, B, use_graph=True, per_row=True, shared_prompt=True, max_new=need) if shared
           else Decoder(model, B, use_graph=True, per_row=True))
    kw = dict(temperature=0.8, **SMP, decoder=dec, shared_prompt=shared)
    evs = []
    admit, first = dec.admit, dec.sample_admitted

    def timed_admit(*args, **kwargs):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        evs.append([e, None])
        return admit(*args, **kwargs)

    def timed_first(*args, **kwargs):
        first(*args, **kwargs)
        evs[-1][1] = torch.cuda.Event(enable_timing=True)
        evs[-1][1].record()

    dec.admit, dec.sample_admitted = timed_admit, timed_first
    chunks = [range(i, min(i + B, len(prompts))) for i in range(0, len(prompts), B)]

    def go(ps, bs):
        if serve:
            model.generate_batch(ps, bs, batch_size=B, **kw)
            return dec.queue_stats["steps"], dec.queue_stats["admissions"]
        mine = [c for c in chunks if c[-1] < len(ps)]
        for ch in mine:
            model.generate_batch([ps[i] for i in ch], max(bs[i] for i in ch), **kw)
        return sum(max(bs[i] for i in ch) - 1 for ch in mine), len(mine)

    go(prompts[:2 * B], [3] * (2 * B))  # warm-up: tuner, allocator, graph capture
    del evs[:]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps, admissions = go(prompts, budgets)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    adm = sum(a.elapsed_time(b) for a, b in evs) * 1e-3
    dec.release()
    return dt, steps, admissions, adm


def run_recompute(model, idx, new):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    model.generate(idx, new, temperature=0.8, **SMP)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="gpt2,gpt2-xl")
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--prompt", type=int, default=128)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--recompute-new", type=int, default=32, help="tokens timed for the recompute loop (slow)")
    ap.add_argument("--modes", default="recompute,cached,graph", help="of recompute, cached, graph, rows")
    ap.add_argument("--ragged", action="store_true", help="add mode 'ragged': unequal prompt lengths, per-row graph")
    ap.add_argument("--repeat", type=int, default=1, help="run the mode list this many times (interleaved)")
    ap.add_argument("--samples", type=int, default=0, help="also time N samples of one prompt: loop vs one batch")
    ap.add_argument("--calibrate", action="store_true", help="first print the box calibration GEMM (utils/boxcal.py)")
    ap.add_argument("--quantize", default="", choices=["", "int8"],
                    help="int8: add int8 weight-only twins of the graph and rows modes (graph_int8, rows_int8)")
    ap.add_argument("--kv_quantize", default="", choices=["", "int8"],
                    help="int8: add int8-KV-cache twins of the graph and rows modes (graph_kv8, rows_kv8; with "
                         "--quantize int8 also graph_int8_kv8, rows_int8_kv8)")
    ap.add_argument("--shared_prompt", action="store_true",
                    help="add shared-prompt twins of the rows modes (rows_shared, rows_int8_shared), ttft_ms on both, "
                         "and sample_batch_shared with --samples")
    ap.add_argument("--shared_prefix", action="store_true",
                    help="time prompts of one --prompt-token prefix + unequal suffixes (--suffix): the unshared "
                         "per-row decoder (prefix_rows) against the shared-prefix one (prefix_shared), ttft_ms on both")
    ap.add_argument("--suffix", type=int, default=32, help="--shared_prefix: the longest suffix (1 .. N over the batch)")
    ap.add_argument("--queue", type=int, default=0,
                    help="time R requests of unequal budgets (--budgets) in chunks of B (queue_chunks) against one "
                         "queue through B refilled rows (queue_serve); with --shared_prompt their _shared twins")
    ap.add_argument("--budgets", default="16:256", help="--queue: new tokens per request, uniform in LO:HI")
    ap.add_argument("--memory", action="store_true", help="add each run's peak allocated bytes (decoder_peak_mb)")
    ap.add_argument("--speculate", default="", help="K[,K ...]: add speculative twins of the rows modes (rows_specK)")
    ap.add_argument("--spec_ngram", type=int, default=3, help="--speculate: the longest n-gram looked up")
    ap.add_argument("--spec_table", default="", help="right, wrong or both: add table-drafted twins "
                                                     "(rows_specK_right: all accepted, rows_specK_wrong: none)")
    ap.add_argument("--penalties", default="", help="RP,PP,FP: add penalised twins of the graph and rows modes "
                                                    "(graph_pen, rows_pen) on a Decoder(penalize=True)")
    ap.add_argument("--logprobs", default="", help="N[,N ...]: add twins of the graph and rows modes that record "
                                                   "log-probabilities and N alternatives (graph_lpN, rows_lpN)")
    ap.add_argument("--top_k", type=int, default=200, help="0: no top-k")
    ap.add_argument("--top_p", type=float, default=1.0, help="nucleus mass; 1.0: off")
    ap.add_argument("--min_p", type=float, default=0.0, help="floor relative to the most likely token; 0.0: off")
    a = ap.parse_args()
    SMP.update(top_k=a.top_k, top_p=a.top_p if a.top_p < 1.0 else None, min_p=a.min_p if a.min_p > 0.0 else None)
    extra = {k: v for k, v in (("top_k", a.top_k), ("top_p", a.top_p), ("min_p", a.min_p))
             if v != ap.get_default(k)}  # the default run prints what it always did
    cal = None
    if a.calibrate or a.queue:
        from nanosandbox_amd.utils.boxcal import calibration_gemm
        cal = calibration_gemm()
        print(json.dumps({"calibration_gemm": cal}), flush=True)
    modes = a.modes.split(",") + (["ragged"] if a.ragged else [])
    modes = [m for m in modes if m]
    if a.quantize:  # each int8 twin right after its bf16 mode
        modes = [t for m in modes for t in ([m, f"{m}_{a.quantize}"] if m in ("graph", "rows") else [m])]
    if a.kv_quantize:  # each int8-cache twin right after its mode (the int8-weight twins included)
        modes = [t for m in modes for t in ([m, f"{m}_kv8"] if m.partition("_")[0] in ("graph", "rows") else [m])]
    if a.shared_prompt:  # each shared twin right after its rows mode (bf16 caches only)
        modes = [t for m in modes for t in ([m, f"{m}_shared"] if m in ("rows", "rows_int8") else [m])]
    if a.speculate:  # the speculative twins right after their rows mode (bf16 caches only)
        twins = [f"spec{int(k)}" + t for k in a.speculate.split(",")
                 for t in [""] + ["_" + x for x in a.spec_table.split(",") if x]]
        modes = [t for m in modes for t in ([m] + [f"{m}_{x}" for x in twins] if m in ("rows", "rows_int8") else [m])]
    if a.penalties:  # each penalised twin right after its mode
        rp, pp, fp = (float(x) for x in a.penalties.split(","))
        PEN.update(repetition_penalty=rp, presence_penalty=pp, frequency_penalty=fp)
        extra["penalties"] = a.penalties
        modes = [t for m in modes for t in ([m, f"{m}_pen"] if m in ("graph", "rows") else [m])]
    if a.logprobs:  # the recording twins right after their mode
        twins = [f"lp{int(n)}" for n in a.logprobs.split(",")]
        modes = [t for m in modes for t in ([m] + [f"{m}_{x}" for x in twins] if m in ("graph", "rows") else [m])]
    if a.shared_prefix:
        modes = ["prefix_rows", "prefix_shared"]
    block_size = GPTConfig().block_size
    if a.queue:
        lo, hi = (int(x) for x in a.budgets.split(":"))
        if a.queue < 1 or not 1 <= lo <= hi or a.prompt + hi > block_size:
            ap.error(f"--queue needs 1 <= LO <= HI and --prompt + HI <= block_size ({block_size})")
        sfx = "_shared" if a.shared_prompt else ""
        modes = ["queue_chunks" + sfx, "queue_serve" + sfx]
        budgets = queue_budgets(a.queue, lo, hi)
    if a.shared_prefix and (a.suffix < 1 or a.prompt + a.suffix + a.new >= block_size):
        ap.error(f"--prompt + --suffix + --new must stay below block_size ({block_size})")
    if not a.queue and any(m != "recompute" for m in modes) and a.prompt + a.new >= block_size:
        # a cached run feeds positions prompt .. prompt + new (one capture step, then --new timed
        # ones); the position table and the caches end at block_size - 1
        ap.error(f"--prompt + --new must stay below block_size ({block_size}): the last fed position is their sum")
    modes = modes * a.repeat
    for name in a.models.split(","):
        L, H, C = DIMS[name]
        torch.manual_seed(0)
        model = GPT(GPTConfig(n_layer=L, n_head=H, n_embd=C, dropout=0.0, bias=True)).eval().cuda()
        model.set_compute_dtype(torch.bfloat16)
        for B in [int(b) for b in a.batches.split(",")]:
            idx = torch.randint(0, 50257, (B, a.prompt), device="cuda")
            with torch.no_grad():
                for mode in modes if a.queue else []:
                    shared = mode.endswith("_shared")
                    reqs = torch.randint(0, 50257, (a.queue, a.prompt), device="cuda")
                    prompts = [reqs[0] if shared else r for r in reqs]
                    dt, steps, adm, adm_s = run_queue(model, prompts, budgets, B, "serve" in mode, shared)
                    print(json.dumps({"model": name, "batch": B, "mode": mode, "prompt": a.prompt, "requests": a.queue,
                                      "budgets": a.budgets, "new_tokens": sum(budgets),
                                      "tokens_per_s": round(sum(budgets) / dt, 1), "seconds": round(dt, 3),
                                      "steps": steps, "admissions": adm, "admit_share": round(adm_s / dt, 4),
                                      "calibration_tflops": cal.get("tflops"), **extra}), flush=True)
                for mode in [] if a.queue else modes:
                    base, *sfx = mode.split("_")  # graph_int8_kv8 -> graph, int8 weights, int8 caches
                    qz = "int8" if "int8" in sfx else None
                    kvq = "int8" if "kv8" in sfx else None
                    ttft = {}
                    spec = next((int(x[4:]) for x in sfx if x.startswith("spec")), 0)
                    lp = next((int(x[2:]) for x in sfx if x.startswith("lp")), None)
                    if a.memory:
                        torch.cuda.synchronize()
                        torch.cuda.reset_peak_memory_stats()
                        mem0 = torch.cuda.memory_allocated()
                    if base == "prefix":
                        n = a.new
                        lens = suffix_lengths(B, a.suffix)
                        suf = torch.randint(0, 50257, (B, a.suffix), device="cuda")
                        run_prefix(model, idx[0], suf, lens, 4, "shared" in sfx)
                        dt, t1, t2 = run_prefix(model, idx[0], suf, lens, n, "shared" in sfx)
                        ttft = {"ttft_ms": round(t1 * 1e3, 3), "suffix": a.suffix}
                        if t2 is not None:
                            ttft["ttft_cached_ms"] = round(t2 * 1e3, 3)
                    elif spec:
                        n = a.new
                        table = next((x for x in sfx if x in ("right", "wrong")), None)
                        dt, st = run_spec(model, idx, n, spec, a.spec_ngram, table, qz)
                        ttft = {"steps": st["steps"], "accepted": sum(st["accepted"]), "offered": sum(st["offered"]),
                                "acceptance": round(sum(st["accepted"]) / max(1, sum(st["offered"])), 4)}
                    elif base in ("rows", "ragged"):
                        n = a.new
                        lens = ragged_lengths(B, a.prompt) if base == "ragged" else None
                        run_rows(model, idx, 4, lens, qz, kvq, "shared" in sfx, "pen" in sfx, lp)
                        dt, t1 = run_rows(model, idx, n, lens, qz, kvq, "shared" in sfx, "pen" in sfx, lp)
                        if a.shared_prompt:
                            ttft = {"ttft_ms": round(t1 * 1e3, 3)}
                    elif mode == "recompute":
                        run_recompute(model, idx, 2)  # warm-up (tuner, allocator)
                        n = a.recompute_new
                        dt = run_recompute(model, idx, n)
                    else:
                        n = a.new
                        run_cached(model, idx, 4, base == "graph", qz, kvq, "pen" in sfx, lp)
                        dt = run_cached(model, idx, n, base == "graph", qz, kvq, "pen" in sfx, lp)
                    mem = ({"decoder_peak_mb": round((torch.cuda.max_memory_allocated() - mem0) / 2 ** 20, 1)}
                           if a.memory else {})
                    print(json.dumps({"model": name, "batch": B, "mode": mode, "prompt": a.prompt, "new_tokens": n,
                                      "tokens_per_s": round(B * n / dt, 1), "ms_per_token": round(dt / n * 1e3, 3),
                                      **ttft, **mem, **extra}),
                          flush=True)
        if a.samples:
            prompt = torch.randint(0, 50257, (a.prompt,), device="cuda")
            with torch.no_grad():
                flows = [(False, False), (True, False)] + ([(True, True)] if a.shared_prompt else [])
                for batched, shared in flows * a.repeat:
                    run_samples(model, prompt, a.samples, 4, batched, shared)  # warm-up (tuner, allocator)
                    dt = run_samples(model, prompt, a.samples, a.new, batched, shared)
                    print(json.dumps({"model": name, "samples": a.samples, "new_tokens": a.new, "prompt": a.prompt,
                                      "mode": ("sample_batch_shared" if shared else "sample_batch") if batched
                                      else "sample_loop",
                                      "tokens_per_s": round(a.samples * a.new / dt, 1), "seconds": round(dt, 3),
                                      **extra}),
                          flush=True)
        del model
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
