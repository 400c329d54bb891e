"""What the decode runtime launches and what it produces, per mode, pinned to a recorded run (GPU).

``tests/golden/decode_launches.json`` (``scripts/record_decode_launches.py``, recorded on an MI355X with
the ``runtime/decode.py`` of the commit to compare against, never with the tree under test) holds for
every case of ``CASES``

* the names of the kernel-library calls of an eager run (``use_graph=False``): the prefill, the first
  draw and two steps (the queue: its whole run), and
* from a run on captured graphs: the new tokens, the keys of ``Decoder.sgraphs``, ``Decoder.replays``
  and, where the mode has them, ``queue_stats``, ``spec_stats`` and the bits of the recorded
  log-probabilities.

The Python that drives the kernels may be rearranged freely; these may not move.  Everything goes
through the public front ends and ``Decoder``'s public methods, so one file observes any tree.
"""

import contextlib
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_launches.json")
ARGS = dict(block_size=64, vocab_size=97, n_layer=2, n_head=2, n_embd=128, bias=True, dropout=0.0)
NEW = 6
SAMPLING = dict(temperature=0.8, top_k=20)
PEN = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1)
UNPINNED_TOKENS = ()  # cases whose tokens two recordings of one commit disagreed on: launches only


def _tokens(*ids):
    return torch.tensor(ids, dtype=torch.int64)


PROMPT = _tokens(5, 9, 2, 44, 7, 1, 30, 8, 61)
RAGGED = [PROMPT, _tokens(12, 3, 77, 5, 20), _tokens(*range(40, 52))]
QUEUE = RAGGED + [_tokens(8, 8, 1, 2, 3, 4, 5), _tokens(90, 2, 14, 6, 33, 21, 70, 11)]
BUDGETS = [6, 2, 5, 3, 6]
SYSTEM = _tokens(4, 17, 60, 2, 35, 9)
PREFIXED = [torch.cat([SYSTEM, _tokens(*s)]) for s in ((1, 50, 3, 8, 22), (2, 6, 13), (3, 71, 4, 19, 28, 5))]
REPEATING = [_tokens(7, 8, 9, 7, 8, 9, 7, 8), _tokens(3, 3, 3, 3, 3, 3)]  # n-gram drafts have something to find
TABLE = [(torch.arange(ARGS["block_size"] + 1) * 7 + b) % ARGS["vocab_size"] for b in range(2)]

# case -> (front end, its prompts: a row count of PROMPT or a list, the keywords that choose the decoder
# (the ``*_decoder`` builders take them too), the keywords of the call alone)
CASES = {
    "plain_b1": ("cached", 1, {}, {}),
    "plain_b3": ("cached", 3, {}, {}),
    "per_row_stop_b3": ("batch", RAGGED, {}, dict(stop_token=3)),
    "int8_b1": ("cached", 1, dict(quantize="int8"), {}),
    "int8_b3": ("cached", 3, dict(quantize="int8"), {}),
    "kv8_b3": ("cached", 3, dict(kv_quantize="int8"), {}),
    "shared_prompt_b3": ("cached", 3, dict(shared_prompt=True), {}),
    "shared_prefix": ("batch", PREFIXED, dict(shared_prefix=True), dict(stop_token=3)),
    "queue": ("batch", QUEUE, dict(batch_size=2), dict(stop_token=3)),
    "spec2_ngram_b2": ("batch", REPEATING, dict(speculate=2), {}),
    "spec2_table_b2": ("batch", REPEATING, dict(speculate=2), dict(spec_table=TABLE)),
    "penalize_off": ("decoder", 3, dict(penalize=True), {}),
    "penalize_on": ("cached", 3, dict(PEN), {}),
    "logprobs2": ("cached", 3, dict(logprobs=2), {}),
    "top_p": ("cached", 3, {}, dict(top_p=0.9)),
    "pen_lp": ("batch", RAGGED, dict(PEN, logprobs=2), dict(stop_token=3)),
}


def build_model():
    from nanosandbox_amd.models import GPT, GPTConfig

    torch.manual_seed(0)
    return GPT(GPTConfig(**ARGS)).eval().cuda().set_compute_dtype(torch.bfloat16)


@contextlib.contextmanager
def _record():
    """The names of the kernel-library calls made inside the block."""
    from nanosandbox_amd.ops import functional

    calls = []
    real_call = functional._lib.call
    functional._lib.call = lambda name, *a: (calls.append(name), real_call(name, *a))[1]
    try:
        yield calls
    finally:
        functional._lib.call = real_call


def _bits(rec):
    return [t.contiguous().view(torch.int32).tolist() if t.dtype == torch.float32 else t.tolist() for t in rec]


def _run(model, name, new, use_graph):
    """One run of the case -> (new tokens per row, the decoder's state after it, the records or None)."""
    from nanosandbox_amd.runtime.decode import Decoder, batch_decoder, cached_decoder

    front, prompts, mode, call = CASES[name]
    torch.manual_seed(1234)  # the decoder's salt, then the call's
    if front == "decoder":  # a mode no front end asks for: a penalising decoder and no penalty passed
        idx = PROMPT[None].repeat(prompts, 1).cuda()
        dec = Decoder(model, prompts, use_graph=use_graph, **mode)
        dec.reseed()
        dec.sample_into(dec.prefill(idx), **SAMPLING)
        dec.run(new - 1, **SAMPLING)
        out, T0 = dec.gen[:, :idx.shape[1] + new].tolist(), idx.shape[1]
    elif front == "cached":
        idx = PROMPT[None].repeat(prompts, 1).cuda()
        dec = cached_decoder(model, idx, new, use_graph=use_graph, **mode)
        out, T0 = model.generate_cached(idx, new, decoder=dec, **SAMPLING, **mode, **call), idx.shape[1]
    else:
        budget = BUDGETS if name == "queue" and new == NEW else new
        dec = batch_decoder(model, prompts, budget, use_graph=use_graph, **mode)
        out, T0 = model.generate_batch(prompts, budget, decoder=dec, **SAMPLING, **mode, **call), None
    rec = None
    if mode.get("logprobs") is not None:
        out, rec = out
        rec = _bits(rec) if front == "cached" else [_bits(r) for r in rec]
    if T0 is None:
        news = [y.tolist()[p.numel():] for y, p in zip(out, prompts)]
    else:
        news = [row[T0:] for row in (out if isinstance(out, list) else out.tolist())]
    state = dict(graphs=sorted(map(repr, dec.sgraphs)), replays=dec.replays)
    if mode.get("batch_size"):
        state["queue_stats"] = dict(dec.queue_stats)
    if dec.K:
        state["spec_stats"] = dec.spec_stats
    dec.release()
    return news, state, rec


def observe(model, name) -> dict:
    """Everything the fixture holds for a case, from this tree."""
    with _record() as calls:
        # prefill, first draw and two steps; the queue's eager run is its whole schedule
        _run(model, name, NEW if name == "queue" else 3, use_graph=False)
    seen = dict(launches=list(calls))
    news, state, rec = _run(model, name, NEW, use_graph=True)
    seen.update(tokens=news, **state)
    if rec is not None:
        seen["lp"] = rec
    return seen


@pytest.fixture(scope="module")
def model(kernels):
    return build_model()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)
    assert doc["model"] == ARGS and sorted(doc["cases"]) == sorted(CASES)
    return doc["cases"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_launches_tokens_and_graph_keys_are_the_recorded_ones(model, golden, name):
    want, got = golden[name], observe(model, name)
    assert got["replays"] > 0  # the run was on the decoder that was looked at
    assert got["launches"] == want["launches"]
    assert got["graphs"] == want["graphs"]
    assert got["replays"] == want["replays"]
    for key in ("queue_stats", "spec_stats"):
        assert got.get(key) == want.get(key), key
    if name not in UNPINNED_TOKENS:
        assert got["tokens"] == want["tokens"]
        assert got.get("lp") == want.get("lp")
    assert ("tokens" in want) == (name not in UNPINNED_TOKENS)
