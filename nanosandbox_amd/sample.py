"""Sampling CLI (nanoGPT ``sample.py`` contract).

    python sample.py --out_dir=out-shakespeare-char --start="ROMEO:" --num_samples=3 --max_new_tokens=200

Loads ``<out_dir>/ckpt.pt`` (``init_from='resume'``) or GPT-2 weights from a
local HF snapshot (``init_from='gpt2*'``).  Text codec: the dataset's
``meta.json``/``meta.pkl`` for char models, else tiktoken / a local HF GPT-2
tokenizer when available, else raw token ids (``--start="11,42,7"``).
On MI355X the forward runs the same HIP kernels as training; with ``kv_cache=True``
(default) each new token runs one position through the model against per-layer
KV caches, replayed as a HIP graph (``runtime/decode.py``).  ``--sample_batch=N`` generates N
samples of the prompt per decoder run, ``--prompts_file=FILE`` one prompt per line as a
batch of unequal lengths, ``--stop_token=ID`` ends a sample at that token
(``GPT.generate_batch``: one position and one finished flag per row on the device).
``--top_p=0.9`` (nucleus) and ``--min_p=0.05`` narrow the sampled set on top of ``top_k``
(``--top_k=0``: no top-k); on the GPU the selection runs inside the sampling kernel.
``--quantize=int8`` decodes with int8 weight-only linears (per-row scales; the KV-cache
path only, so it refuses ``--kv_cache=False``).  ``--kv_quantize=int8`` keeps the KV caches
as int8 rows with one scale each (the same refusal).  ``--shared_prompt=True`` with
``--sample_batch=N`` encodes and caches the prompt once for the N rows of a batch and once
for all rounds (``Decoder(shared_prompt=True)``); it refuses ``--prompts_file``,
``--kv_cache=False`` and ``--kv_quantize``.  ``--shared_prefix=True`` is the same for prompts that
share only a prefix (``--prompts_file``: a system prompt followed by different questions): the
longest common token prefix is encoded and cached once for the batch and for all rounds, and
every row prefills only what it adds (``Decoder.prefill_suffixes``); it refuses
``--kv_cache=False``, ``--kv_quantize`` and ``--shared_prompt``.  ``--serve_batch=N`` serves all
requests (``num_samples`` rounds of the prompts file, or ``num_samples`` copies of ``start``) as one
queue through N decoder rows, a finished row taking the next request (``Decoder.serve``), and prints
the results in request order; it needs the KV-cache path, refuses ``--shared_prefix`` and composes
with ``--shared_prompt``, ``--quantize``, ``--kv_quantize`` and ``--stop_token``.
``--speculate=K`` (1 .. 7) decodes speculatively: every model pass feeds a row's token and K
continuations guessed by ``--spec_ngram=N``-gram lookup in the row's own text and keeps those the
model itself draws (``Decoder(speculate=K)``): the same samples for the same seed, up to K + 1
tokens per pass.  It needs the KV-cache path, refuses ``--kv_quantize``, ``--shared_prompt``,
``--shared_prefix`` and ``--serve_batch`` and composes with ``--quantize``, ``--stop_token``,
``--top_p`` / ``--min_p``, ``--sample_batch`` and ``--prompts_file`` (rows * (K + 1) <= 16 on the GPU).
``--repetition_penalty=1.3`` (> 0; divides the positive and multiplies the negative logits of the ids a
sample's text already holds), ``--presence_penalty=0.5`` (subtracted from them once) and
``--frequency_penalty=0.2`` (subtracted once per occurrence) discourage a sample from repeating itself
(``ops.penalize_logits``: prompt and generated tokens count); on the GPU they are applied inside the
sampling kernel's launch (``Decoder(penalize=True)``).  They compose with every mode but ``--speculate``.
``--logprobs=N`` (0 .. 8; -1: off) prints under each sample the summed log-probability of its new tokens
under the model's own distribution (the raw logits, before penalties, temperature and filters) and their
perplexity, and with N > 0 every new token with its N most likely alternatives
(``Decoder(logprobs=N)``: recorded by one more launch inside the decode step); every mode but
``--speculate``.  ``--score=True`` with ``--prompts_file`` generates nothing: every line is scored
(``GPT.score``) and printed with its summed log-probability, token count and perplexity.
"""

from __future__ import annotations

import os
import sys

import torch

from .config import parse_argv
from .data import load_meta, resolve_data_dir
from .models import GPT, GPTConfig
from .ops import check_logprobs, check_sampling_filters, check_sampling_penalties
from .utils import load_checkpoint, load_model_state

SAMPLE_DEFAULTS = dict(
    init_from="resume",  # 'resume' (from out_dir) or a gpt2 variant (e.g. 'gpt2-xl')
    out_dir="out",
    start="\n",  # or "<|endoftext|>" or etc. Can also specify a file, use as: "FILE:prompt.txt"
    num_samples=10,
    max_new_tokens=500,
    temperature=0.8,
    top_k=200,  # keep the k most likely tokens; 0: off
    top_p=1.0,  # nucleus: the smallest set of most likely tokens whose mass reaches top_p; 1.0: off
    min_p=0.0,  # drop tokens less likely than min_p times the most likely one; 0.0: off
    repetition_penalty=1.0,  # > 0: logits of ids the text already holds are divided (positive) or multiplied (negative) by it; 1.0: off
    presence_penalty=0.0,  # subtracted from the logit of every id the text already holds; 0.0: off
    frequency_penalty=0.0,  # subtracted from an id's logit once per occurrence in the text; 0.0: off
    seed=1337,
    device="cuda",
    dtype="bfloat16",
    compile=False,
    data_dir="",
    kv_cache=True,  # per-layer KV caches + a replayed HIP-graph decode step (runtime/decode.py); False: nanoGPT's recompute loop
    sample_batch=1,  # samples of the prompt generated per decoder run (num_samples is still the total)
    prompts_file="",  # one prompt per line, generated as one ragged batch per sample round (start is ignored)
    stop_token=-1,  # token id that ends a sample (printed text ends before it); -1: none
    quantize="",  # "int8": int8 weight-only decoding on the KV-cache path (Decoder(quantize="int8")); "": off
    kv_quantize="",  # "int8": int8 KV caches, one scale per cache row (Decoder(kv_quantize="int8")); "": off
    shared_prompt=False,  # sample_batch > 1: encode and cache the prompt once for the batch (Decoder(shared_prompt=True))
    shared_prefix=False,  # prompts_file / sample_batch > 1: encode and cache the prompts' common prefix once for the batch
    serve_batch=0,  # N > 0: all requests as one queue through N decoder rows, finished rows refilled (Decoder.serve); 0: off
    speculate=0,  # K > 0: speculative decoding, K tokens drafted per model pass (Decoder(speculate=K)); 0: off
    spec_ngram=3,  # speculate: the longest n-gram looked up in the row's own text for a draft
    logprobs=-1,  # N >= 0: print each sample's log-probability and perplexity, N > 0 (<= 8): and N alternatives per token; -1: off
    score=False,  # with prompts_file: score every line (GPT.score) instead of generating
)


def _penalties(c) -> dict:
    """The three penalty keys as the front ends' keywords."""
    return {k: c[k] for k in ("repetition_penalty", "presence_penalty", "frequency_penalty")}


def _logprobs(c) -> dict:
    """The ``logprobs`` keyword of the front ends (off: none, and they return the tokens alone)."""
    return dict(logprobs=c["logprobs"]) if c["logprobs"] >= 0 else {}


def _print_logprobs(rec, new, decode):
    """Under a sample: the summed log-probability and perplexity of the ``new`` tokens that were printed
    (``rec``: their ``ops.LogProbs``, possibly longer: a stop token is not printed), then every token
    with its alternatives."""
    n = len(new)
    if not n:
        return
    tok = rec.token[:n].double()
    print(f"logprob {float(tok.sum()):.4f} over {n} tokens, perplexity {float(torch.exp(-tok.mean())):.4f}")
    if rec.top_ids.shape[-1]:
        for i, t in enumerate(new):
            alts = ", ".join(f"{decode([a])!r} {lp:.3f}" for a, lp in zip(rec.top_ids[i].tolist(), rec.top[i].tolist())
                             if a >= 0)
            print(f"  {decode([t])!r} {float(rec.token[i]):.3f} | {alts}")


def _score_file(model, c, encode, device):
    """score: every line of prompts_file through ``GPT.score`` as one right-padded batch."""
    with open(c["prompts_file"], "r", encoding="utf-8") as f:
        texts = [ln.rstrip("\n") for ln in f if ln.strip()]
    ids = [encode(t) for t in texts]
    if min(len(i) for i in ids) < 2:
        raise ValueError("--score needs at least 2 tokens per line: the first token is given, not predicted")
    idx = torch.zeros(len(ids), max(len(i) for i in ids), dtype=torch.long, device=device)
    for b, i in enumerate(ids):
        idx[b, :len(i)] = torch.tensor(i, dtype=torch.long)
    rec = model.score(idx, lengths=[len(i) for i in ids], top=max(c["logprobs"], 0))
    outs = []
    for b, (t, i) in enumerate(zip(texts, ids)):
        tok = rec.token[b, :len(i) - 1].double()
        outs.append((float(tok.sum()), len(i) - 1, float(torch.exp(-tok.mean()))))
        print(t)
        print(f"logprob {outs[-1][0]:.4f} over {outs[-1][1]} tokens, perplexity {outs[-1][2]:.4f}")
        print("---------------")
    return outs


def _serve_queue(model, c, encode, decode, start, device):
    """serve_batch: every request (num_samples rounds of the prompts file, or num_samples copies
    of start) through one queue of ``serve_batch`` rows (``GPT.generate_batch(batch_size=)``)."""
    stop = c["stop_token"] if c["stop_token"] >= 0 else None
    if c["prompts_file"]:
        with open(c["prompts_file"], "r", encoding="utf-8") as f:
            texts = [ln.rstrip("\n") for ln in f if ln.strip()] * c["num_samples"]
    else:
        texts = [start] * c["num_samples"]
    prompts = [torch.tensor(encode(t), dtype=torch.long, device=device) for t in texts]
    ys = model.generate_batch(prompts, c["max_new_tokens"], temperature=c["temperature"], top_k=c["top_k"],
                              stop_token=stop, top_p=c["top_p"], min_p=c["min_p"], quantize=c["quantize"] or None,
                              kv_quantize=c["kv_quantize"] or None, shared_prompt=bool(c["shared_prompt"]),
                              batch_size=c["serve_batch"], **_penalties(c), **_logprobs(c))
    ys, recs = ys if _logprobs(c) else (ys, None)
    outs = []
    for i, (p, y) in enumerate(zip(prompts, ys)):
        new = y[p.numel():].tolist()
        if stop is not None and stop in new:
            new = new[:new.index(stop)]
        outs.append(decode(p.tolist() + new))
        print(outs[-1])
        if recs is not None:
            _print_logprobs(recs[i], new, decode)
        print("---------------")
    return outs


def _generate_batches(model, c, encode, decode, start, device):
    """sample_batch / prompts_file / stop_token: batches of prompts through
    ``GPT.generate_batch`` (one per_row decoder per batch size, kept across batches)."""
    stop = c["stop_token"] if c["stop_token"] >= 0 else None
    quantize = c["quantize"] or None
    kv_quantize = c["kv_quantize"] or None
    shared = bool(c["shared_prompt"])  # main() has refused prompts_file, kv_cache=False and kv_quantize with it
    prefix = bool(c["shared_prefix"])  # main() has refused kv_cache=False, kv_quantize and shared_prompt with it
    if c["prompts_file"]:
        with open(c["prompts_file"], "r", encoding="utf-8") as f:
            texts = [ln.rstrip("\n") for ln in f if ln.strip()]
        batches = [texts] * c["num_samples"]  # every sample round: all prompts as one ragged batch
    else:
        n, sb = c["num_samples"], max(1, c["sample_batch"])
        batches = [[start] * min(sb, n - i) for i in range(0, n, sb)]
    decs, outs = {}, []
    try:
        for batch in batches:
            prompts = [torch.tensor(encode(t), dtype=torch.long, device=device) for t in batch]
            if c["kv_cache"]:
                from .runtime.decode import batch_decoder
                B = len(prompts)
                mode = dict(quantize=quantize, kv_quantize=kv_quantize, shared_prompt=shared, shared_prefix=prefix)
                if c["speculate"]:
                    mode.update(speculate=c["speculate"], spec_ngram=c["spec_ngram"])
                mode.update(_penalties(c))
                mode.update(_logprobs(c))
                if B not in decs:  # a shared prompt / prefix stays cached in it: later rounds do not encode it again
                    decs[B] = batch_decoder(model, prompts, c["max_new_tokens"], **mode)
                ys = model.generate_batch(prompts, c["max_new_tokens"], temperature=c["temperature"], top_k=c["top_k"],
                                          stop_token=stop, decoder=decs[B], top_p=c["top_p"], min_p=c["min_p"], **mode)
                ys, recs = ys if _logprobs(c) else (ys, None)
            else:
                ys = [model.generate(p[None], c["max_new_tokens"], temperature=c["temperature"], top_k=c["top_k"],
                                     top_p=c["top_p"], min_p=c["min_p"], **_penalties(c), **_logprobs(c))
                      for p in prompts]
                recs = [type(r)(*(t[0] for t in r)) for _, r in ys] if _logprobs(c) else None
                ys = [(y[0] if _logprobs(c) else y)[0] for y in ys]
            for i, (p, y) in enumerate(zip(prompts, ys)):
                new = y[p.numel():].tolist()
                if stop is not None and stop in new:
                    new = new[:new.index(stop)]
                text = decode(p.tolist() + new)
                outs.append(text)
                print(text)
                if recs is not None:
                    _print_logprobs(recs[i], new, decode)
                print("---------------")
    finally:
        for d in decs.values():
            d.release()
    return outs


def _codec(checkpoint, data_dir):
    meta = None
    if checkpoint is not None and "config" in checkpoint and "dataset" in checkpoint["config"]:
        meta = load_meta(resolve_data_dir(checkpoint["config"]["dataset"], data_dir or
                                          checkpoint["config"].get("data_dir", "")))
    if meta is not None:
        print("Loading meta for char codec")
        stoi, itos = meta["stoi"], meta["itos"]
        return (lambda s: [stoi[c] for c in s]), (lambda ids: "".join(itos[i] for i in ids))
    try:
        import tiktoken
        enc = tiktoken.get_encoding("gpt2")
        return (lambda s: enc.encode(s, allowed_special={"<|endoftext|>"})), enc.decode
    except Exception:
        pass
    try:
        from transformers import GPT2TokenizerFast
        tok = GPT2TokenizerFast.from_pretrained(os.environ.get("NSA_HF_GPT2_DIR", "gpt2"), local_files_only=True)
        return tok.encode, tok.decode
    except Exception:
        print("no GPT-2 tokenizer available offline: prompts/outputs are raw token ids")
        return (lambda s: [int(t) for t in s.split(",") if t.strip()]), (lambda ids: ",".join(map(str, ids)))


def main(argv=None):
    c = parse_argv(SAMPLE_DEFAULTS, sys.argv[1:] if argv is None else argv)
    check_sampling_filters(c["top_p"], c["min_p"])
    check_sampling_penalties(c["repetition_penalty"], c["presence_penalty"], c["frequency_penalty"])
    if c["quantize"] not in ("", "int8"):
        raise ValueError(f"quantize must be '' or 'int8', got {c['quantize']!r}")
    if c["quantize"] and not c["kv_cache"]:
        raise ValueError("--quantize needs the KV-cache path: the recompute loop (--kv_cache=False) runs the "
                         "unquantized model")
    if c["kv_quantize"] not in ("", "int8"):
        raise ValueError(f"kv_quantize must be '' or 'int8', got {c['kv_quantize']!r}")
    if c["kv_quantize"] and not c["kv_cache"]:
        raise ValueError("--kv_quantize needs the KV-cache path: the recompute loop (--kv_cache=False) has no "
                         "cache to quantize")
    if c["shared_prompt"]:
        if c["prompts_file"]:
            raise ValueError("--shared_prompt shares one prompt among the rows of a batch: it cannot be combined "
                             "with --prompts_file (different prompts)")
        if not c["kv_cache"]:
            raise ValueError("--shared_prompt needs the KV-cache path: the recompute loop (--kv_cache=False) has no "
                             "cache to share")
        if c["kv_quantize"]:
            raise ValueError("--shared_prompt keeps bf16 caches: it cannot be combined with --kv_quantize")
    if c["shared_prefix"]:
        if c["shared_prompt"]:
            raise ValueError("--shared_prefix and --shared_prompt are two forms of sharing: pass one of them")
        if not c["kv_cache"]:
            raise ValueError("--shared_prefix needs the KV-cache path: the recompute loop (--kv_cache=False) has no "
                             "cache to share")
        if c["kv_quantize"]:
            raise ValueError("--shared_prefix keeps bf16 caches: it cannot be combined with --kv_quantize")
    if c["logprobs"] != -1:
        check_logprobs(c["logprobs"])
        if c["speculate"]:
            raise ValueError("--logprobs cannot be combined with --speculate: a verified position can be written by "
                             "more than one step")
    if c["score"] and not c["prompts_file"]:
        raise ValueError("--score scores the lines of --prompts_file: pass one")
    if c["serve_batch"] < 0:
        raise ValueError(f"serve_batch must be >= 0, got {c['serve_batch']}")
    if c["serve_batch"]:
        if not c["kv_cache"]:
            raise ValueError("--serve_batch refills the rows of a KV-cache decoder: it cannot be combined with "
                             "--kv_cache=False")
        if c["shared_prefix"]:
            raise ValueError("--serve_batch cannot admit suffixes against a shared prefix yet: it cannot be combined "
                             "with --shared_prefix")
    if c["speculate"]:
        from .runtime.decode import _check
        _check(None, c["kv_quantize"] or None, c["shared_prompt"], c["shared_prefix"], bool(c["serve_batch"]),
               c["speculate"], c["spec_ngram"])
        if not c["kv_cache"]:
            raise ValueError("--speculate needs the KV-cache path: the recompute loop (--kv_cache=False) decodes one "
                             "token per pass")
        if _penalties(c) != dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0):
            raise ValueError("--speculate cannot be combined with --repetition_penalty / --presence_penalty / "
                             "--frequency_penalty: a verified position's counts would have to include its drafts")
    spec = dict(speculate=c["speculate"], spec_ngram=c["spec_ngram"]) if c["speculate"] else {}
    quantize = c["quantize"] or None
    kv_quantize = c["kv_quantize"] or None
    torch.manual_seed(c["seed"])
    device = c["device"]
    if device.startswith("cuda") and not torch.cuda.is_available():
        device = "cpu"
    checkpoint = None
    if c["init_from"] == "resume":
        checkpoint = load_checkpoint(os.path.join(c["out_dir"], "ckpt.pt"), map_location="cpu")
        model = GPT(GPTConfig(**checkpoint["model_args"]))
        load_model_state(model, checkpoint["model"])
    elif c["init_from"].startswith("gpt2"):
        model = GPT.from_pretrained(c["init_from"], dict(dropout=0.0))
    else:
        raise ValueError(c["init_from"])
    model.eval().to(device)
    if device.startswith("cuda"):
        model.set_compute_dtype(torch.bfloat16)
    encode, decode = _codec(checkpoint, c["data_dir"])
    start = c["start"]
    if start.startswith("FILE:"):
        with open(start[5:], "r", encoding="utf-8") as f:
            start = f.read()
    if c["score"]:
        with torch.no_grad():
            return _score_file(model, c, encode, device)
    if c["serve_batch"]:
        with torch.no_grad():
            return _serve_queue(model, c, encode, decode, start, device)
    if c["sample_batch"] > 1 or c["prompts_file"] or c["stop_token"] >= 0:
        with torch.no_grad():
            return _generate_batches(model, c, encode, decode, start, device)
    x = torch.tensor(encode(start), dtype=torch.long, device=device)[None, ...]
    outs = []
    dec = None
    if c["kv_cache"]:
        # one decoder for all samples: weight shadows and the captured step graph are
        # built once, not per sample
        from .runtime.decode import cached_decoder
        dec = cached_decoder(model, x, c["max_new_tokens"], quantize=quantize, kv_quantize=kv_quantize, **spec,
                             **_penalties(c), **_logprobs(c))
    try:
        with torch.no_grad():
            for _ in range(c["num_samples"]):
                if dec is not None:
                    y = model.generate_cached(x, c["max_new_tokens"], temperature=c["temperature"], top_k=c["top_k"],
                                              decoder=dec, top_p=c["top_p"], min_p=c["min_p"], quantize=quantize,
                                              kv_quantize=kv_quantize, **spec, **_penalties(c), **_logprobs(c))
                else:
                    y = model.generate(x, c["max_new_tokens"], temperature=c["temperature"], top_k=c["top_k"],
                                       top_p=c["top_p"], min_p=c["min_p"], **_penalties(c), **_logprobs(c))
                y, rec = y if _logprobs(c) else (y, None)
                text = decode(y[0].tolist())
                outs.append(text)
                print(text)
                if rec is not None:
                    _print_logprobs(type(rec)(*(t[0] for t in rec)), y[0, x.shape[1]:].tolist(), decode)
                print("---------------")
    finally:
        if dec is not None:
            dec.release()
    return outs


if __name__ == "__main__":
    main()
