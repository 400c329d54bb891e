"""The Python that drives the decode kernels (CPU): the one sampling value, the key of a captured
sampling graph, and what the module refuses.

* ``graph_key`` is pinned on a table written out from its rule list (``Decoder.sgraphs`` is read by
  tests and by callers that count captures): the expected tuples are literals, not computed.
* ``sampling`` builds one value however "off" is spelled.
* ``tests/golden/decode_refusals.json`` (``scripts/record_decode_refusals.py``, recorded with the
  ``runtime/decode.py`` of the commit to compare against) holds the exception type and message of every
  single illegal combination in ``VIOLATIONS``, through every door that takes its arguments; they are
  replayed and must be equal.  Two violations passed together must raise ValueError with the message
  of a violation that is present (which one is not pinned: the order of the checks is no contract).
"""

import itertools
import json
import os

import pytest
import torch

from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime import decode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode_refusals.json")
ARGS = dict(block_size=48, vocab_size=97, n_layer=2, n_head=2, n_embd=64, bias=True, dropout=0.0)
NEW = 6


# ---------------------------------------------------------------------------- graph keys

def _key(sampling=(), **mode):
    return decode.graph_key(decode.sampling(**dict(sampling)), **mode)


PEN = dict(repetition_penalty=1.3, presence_penalty=0.2, frequency_penalty=0.1)
S = dict(temperature=0.8, top_k=200)
KEYS = [  # (the sampling settings, the decoder's and the call's part of the key) -> the key
    (dict(temperature=1), {}, (1.0, None)),
    (S, {}, (0.8, 200)),
    (dict(S, top_k=0), {}, (0.8, 0)),  # top_k is stored as given
    (dict(S, top_p=1.0, min_p=0.0, stop_token=-1), {}, (0.8, 200)),  # "off" spelled out: the key of none
    (dict(S, top_p=1.0, min_p=0.0, stop_token=-1), dict(per_row=True), (0.8, 200, None)),
    (S, dict(per_row=True), (0.8, 200, None)),
    (dict(S, stop_token=3), dict(per_row=True), (0.8, 200, 3)),
    (dict(S, top_p=0.9), {}, (0.8, 200, 0.9, None)),  # no per_row, no stop slot
    (dict(S, min_p=0.05), {}, (0.8, 200, None, 0.05)),
    (dict(S, stop_token=3, top_p=0.9, min_p=0.05), dict(per_row=True), (0.8, 200, 3, 0.9, 0.05)),
    (dict(S, stop_token=3), dict(per_row=True, queue=True), (0.8, 200, 3, "queue")),
    (dict(S, top_p=0.9), dict(per_row=True, queue=True), (0.8, 200, None, 0.9, None, "queue")),
    (S, dict(per_row=True, spec=(2, 3)), (0.8, 200, None, "spec", 2, 3)),
    (S, dict(per_row=True, spec=(2, 3), table=True), (0.8, 200, None, "spec", 2, 3, "table")),
    (dict(S, stop_token=3, top_p=0.9), dict(per_row=True, spec=(4, 2)), (0.8, 200, 3, 0.9, None, "spec", 4, 2)),
    (dict(S, stop_token=3, min_p=0.05), dict(per_row=True, spec=(4, 2), table=True),
     (0.8, 200, 3, None, 0.05, "spec", 4, 2, "table")),
    (S, dict(penalize=True), (0.8, 200, "pen", 1.0, 0.0, 0.0)),  # a penalising decoder, no penalty passed
    (dict(S, repetition_penalty=1, presence_penalty=0, frequency_penalty=0), dict(penalize=True),
     (0.8, 200, "pen", 1.0, 0.0, 0.0)),
    (dict(S, **PEN), dict(penalize=True), (0.8, 200, "pen", 1.3, 0.2, 0.1)),
    (dict(S, presence_penalty=1), dict(penalize=True), (0.8, 200, "pen", 1.0, 1.0, 0.0)),
    (S, dict(logprobs=2), (0.8, 200, "lp", 2)),
    (S, dict(logprobs=0), (0.8, 200, "lp", 0)),
    (dict(S, **PEN), dict(penalize=True, logprobs=2), (0.8, 200, "pen", 1.3, 0.2, 0.1, "lp", 2)),  # pen before lp
    (dict(S, stop_token=3, top_p=0.9, **PEN), dict(per_row=True, queue=True, penalize=True, logprobs=0),
     (0.8, 200, 3, 0.9, None, "queue", "pen", 1.3, 0.2, 0.1, "lp", 0)),
]


@pytest.mark.parametrize("sampling,mode,want", KEYS, ids=[repr(k[2]) for k in KEYS])
def test_graph_key(sampling, mode, want):
    got = _key(sampling, **mode)
    assert got == want
    assert [type(x) for x in got] == [type(x) for x in want]  # 1 == 1.0, but the key holds the float


def test_sampling_is_normalised_once_however_off_is_spelled():
    off = decode.sampling(1.0, None, stop_token=-1, top_p=1.0, min_p=0.0, repetition_penalty=1, presence_penalty=0,
                          frequency_penalty=0)
    assert off == decode.sampling()
    assert (off.stop_token, off.top_p, off.min_p, off.penalties) == (None, None, None, None)
    on = decode.sampling(0.8, 200, 3, 0.9, 0.05, **PEN)
    assert tuple(on) == (0.8, 200, 3, 0.9, 0.05, (1.3, 0.2, 0.1))
    assert decode.sampling(presence_penalty=1).penalties == (1.0, 1.0, 0.0)
    # the public normalisers are the same rules
    assert decode.sampling_filters(1.0, 0.0) == (None, None) and decode.sampling_filters(0.9, 0.05) == (0.9, 0.05)
    assert decode.sampling_penalties(1, 0, 0) is None and decode.sampling_penalties(**PEN) == (1.3, 0.2, 0.1)
    for bad in (dict(top_p=0.0), dict(min_p=1.0), dict(repetition_penalty=0.0), dict(presence_penalty=float("inf"))):
        with pytest.raises(ValueError):
            decode.sampling(**bad)


# ---------------------------------------------------------------------------- refusals

def _tokens(*ids):
    return torch.tensor(ids, dtype=torch.int64)


PROMPT = _tokens(5, 9, 2, 44, 7, 1, 30, 8, 61)
RAGGED = [PROMPT, _tokens(12, 3, 77, 5, 20), _tokens(*range(40, 52))]
SAME = [PROMPT] * 3
SYSTEM = _tokens(4, 17, 60, 2, 35, 9)
PREFIXED = [torch.cat([SYSTEM, _tokens(*s)]) for s in ((1, 50, 3, 8, 22), (2, 6, 13), (3, 71, 4, 19, 28, 5, 80))]
IDX = PROMPT[None].repeat(3, 1)
UNEQUAL = torch.stack([PROMPT, PROMPT, PROMPT + 1])
BUDGETS = [6, 2, 5]  # one per prompt: a queue
LONG = 45  # new tokens that do not fit the cache after any of the prompts
INF, NAN = float("inf"), float("nan")

DECODER = ("Decoder",)
CACHED = ("generate_cached", "cached_decoder")
BATCH = ("generate_batch", "batch_decoder")
RUNS = ("generate_cached", "generate_batch")
FRONT = CACHED + BATCH
ALL = DECODER + FRONT


def _v(doors, **kw):
    return {door: dict(kw) for door in doors}


# violation -> door -> the keywords that spell it there (on top of the door's defaults in ``_call``)
VIOLATIONS = {
    "quantize": _v(ALL, quantize="int4"),
    "kv_quantize": _v(ALL, kv_quantize="fp8"),
    "shared_prompt_kv": _v(ALL, shared_prompt=True, kv_quantize="int8"),
    "prefix_and_prompt": _v(BATCH, shared_prefix=True, shared_prompt=True),
    "prefix_kv": _v(BATCH, shared_prefix=True, kv_quantize="int8"),
    "speculate_range": _v(ALL, speculate=8),
    "spec_ngram": _v(ALL, speculate=2, spec_ngram=0),
    "spec_kv": _v(ALL, speculate=2, kv_quantize="int8"),
    "spec_shared_prompt": _v(ALL, speculate=2, shared_prompt=True),
    "spec_shared_prefix": _v(BATCH, speculate=2, shared_prefix=True),
    "spec_queue": _v(BATCH, speculate=2, batch_size=2),
    "spec_budgets": _v(BATCH, speculate=2, max_new_tokens=BUDGETS),
    "spec_penalty": {**_v(DECODER, speculate=2, penalize=True), **_v(FRONT, speculate=2, repetition_penalty=1.3)},
    "spec_presence": _v(FRONT, speculate=2, presence_penalty=0.5),
    "spec_logprobs": _v(ALL, speculate=2, logprobs=2),
    "logprobs_range": _v(ALL, logprobs=9),
    "logprobs_bool": _v(ALL, logprobs=True),
    "shared_one_row": _v(DECODER, shared_prompt=True, batch_size=1),
    "max_new_unshared": _v(DECODER, max_new=4),
    "max_new_range": _v(DECODER, shared_prompt=True, max_new=49),
    "top_p_range": _v(RUNS, top_p=0.0),
    "min_p_range": _v(RUNS, min_p=1.0),
    "repetition_penalty_range": _v(FRONT, repetition_penalty=0.0),
    "presence_penalty_range": _v(FRONT, presence_penalty=INF),
    "frequency_penalty_range": _v(FRONT, frequency_penalty=NAN),
    "prefix_queue": _v(BATCH, shared_prefix=True, batch_size=2),
    "prefix_budgets": _v(BATCH, shared_prefix=True, max_new_tokens=BUDGETS),
    "batch_size_range": _v(BATCH, batch_size=0),
    "budgets_count": _v(BATCH, max_new_tokens=[6, 2]),
    "budgets_range": _v(BATCH, max_new_tokens=[6, 0, 5]),
    "shared_prompt_unequal": {**_v(CACHED, shared_prompt=True, idx=UNEQUAL), **_v(BATCH, shared_prompt=True,
                                                                                  prompts=RAGGED)},
    "shared_prompt_long": _v(FRONT, shared_prompt=True, max_new_tokens=LONG),
    "shared_prefix_long": _v(BATCH, shared_prefix=True, prompts=PREFIXED, max_new_tokens=LONG),
    "quantize_long": _v(CACHED + ("generate_batch",), quantize="int8", max_new_tokens=LONG),
    "kv_quantize_long": _v(CACHED + ("generate_batch",), kv_quantize="int8", max_new_tokens=LONG),
    "speculate_long": _v(CACHED + ("generate_batch",), speculate=2, max_new_tokens=LONG),
}


def build_model():
    torch.manual_seed(0)
    return GPT(GPTConfig(**ARGS)).eval().set_compute_dtype(torch.bfloat16)


@pytest.fixture(scope="module")
def model():
    return build_model()


def _call(model, door, kw):
    """The door with ``kw`` on top of a legal call's arguments."""
    if door == "Decoder":
        return decode.Decoder(model, **{"batch_size": 3, "use_graph": False, **kw})
    if door in CACHED:
        return getattr(decode, door)(model, **{"idx": IDX, "max_new_tokens": NEW, **kw})
    prompts = SAME if kw.get("shared_prompt") else RAGGED  # a legal shared_prompt batch is one prompt
    return getattr(decode, door)(model, **{"prompts": prompts, "max_new_tokens": NEW, **kw})


def refusal(model, door, kw):
    """[exception type, message] of the call, or None if it went through."""
    try:
        out = _call(model, door, kw)
    except Exception as e:  # noqa: BLE001 - the type is what is recorded
        return [type(e).__name__, str(e)]
    if isinstance(out, decode.Decoder):
        out.release()
    return None


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        doc = json.load(f)["cases"]
    assert {k: sorted(v) for k, v in doc.items()} == {k: sorted(v) for k, v in VIOLATIONS.items()}
    return doc


SINGLES = [(name, door) for name, doors in VIOLATIONS.items() for door in doors]


@pytest.mark.parametrize("name,door", SINGLES, ids=[f"{n}-{d}" for n, d in SINGLES])
def test_a_single_violation_is_refused_as_recorded(model, golden, name, door):
    assert refusal(model, door, VIOLATIONS[name][door]) == golden[name][door]
    assert all(getattr(p, "compute", None) is None for p in model.parameters())  # nothing was left behind


def _same(a, b):
    return a is b or (not isinstance(a, (list, torch.Tensor)) and not isinstance(b, (list, torch.Tensor)) and a == b)


def _within(kw, merged):
    return all(k in merged and _same(v, merged[k]) for k, v in kw.items())


def _queue(kw):
    return "batch_size" in kw or not isinstance(kw.get("max_new_tokens", NEW), int)


# what a queue is refused with however it is spelled (``batch_size``, or any list of budgets)
QUEUE_RULES = {"prefix_queue": "shared_prefix", "spec_queue": "speculate"}


def _present(door, merged):
    """The violations the keywords spell: the two of a pair, and any third between them."""
    return [n for n, doors in VIOLATIONS.items() if door in doors and (
        _within(doors[door], merged) or (n in QUEUE_RULES and merged.get(QUEUE_RULES[n]) and _queue(merged)))]


def _pairs():
    for (a, da), (b, db) in itertools.combinations(VIOLATIONS.items(), 2):
        for door in da:
            if door in db and all(_same(v, db[door][k]) for k, v in da[door].items() if k in db[door]):
                yield a, b, door


PAIRS = list(_pairs())


@pytest.mark.parametrize("door", ALL)
def test_two_violations_together_are_refused_with_the_message_of_one_that_is_present(model, golden, door):
    pairs = [(a, b) for a, b, d in PAIRS if d == door]
    assert len(pairs) >= 10
    for a, b in pairs:
        merged = {**VIOLATIONS[a][door], **VIOLATIONS[b][door]}
        present = _present(door, merged)
        assert a in present and b in present
        got = refusal(model, door, merged)
        assert got is not None and got[0] == "ValueError", (a, b, got)
        assert got[1] in [golden[n][door][1] for n in present], (a, b, got)
