"""Which ``Decoder`` a generation call runs on (CPU): a caller's decoder that fits the call's mode is
used and left to the caller, one that does not fit is left alone and a temporary one is built and
released, and the decoders ``sample.py`` keeps across rounds are the ones the calls accept."""

import pytest
import torch

from nanosandbox_amd import sample
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder

NEW = 6
ARGS = dict(block_size=48, vocab_size=97, n_layer=2, n_head=2, n_embd=64, bias=True, dropout=0.0)


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    # bf16 compute: a decoder then owns real weight shadows, which a release would drop
    return GPT(GPTConfig(**ARGS)).eval().set_compute_dtype(torch.bfloat16)


def _tokens(*ids):
    return torch.tensor(ids, dtype=torch.int64)


RAGGED = [_tokens(5, 9, 2, 44, 7, 1, 30, 8, 61), _tokens(12, 3, 77, 5, 20), _tokens(*range(40, 52))]
QUEUE = RAGGED + [_tokens(8, 8, 1, 2, 3, 4, 5), _tokens(90, 2, 14, 6, 33, 21, 70, 11)]
PROMPT = RAGGED[0]
SYSTEM = _tokens(4, 17, 60, 2, 35, 9)
PREFIXED = [torch.cat([SYSTEM, _tokens(*s)]) for s in ((1, 50, 3, 8, 22), (2, 6, 13), (3, 71, 4, 19, 28, 5, 80))]

# front-end path -> (the call, given the model and ``decoder=``; the Decoder arguments that fit it)
PATHS = {
    "cached": (lambda m, d: m.generate_cached(PROMPT[None].repeat(4, 1), NEW, decoder=d), dict(batch_size=4)),
    "cached_shared": (lambda m, d: m.generate_cached(PROMPT[None].repeat(4, 1), NEW, decoder=d, shared_prompt=True),
                      dict(batch_size=4, shared_prompt=True, max_new=NEW)),
    "batch": (lambda m, d: m.generate_batch(RAGGED, NEW, stop_token=3, decoder=d), dict(batch_size=3, per_row=True)),
    "batch_shared": (lambda m, d: m.generate_batch([PROMPT] * 3, NEW, stop_token=3, decoder=d, shared_prompt=True),
                     dict(batch_size=3, per_row=True, shared_prompt=True, max_new=NEW)),
    # the prefix is SYSTEM (the suffixes start differently) and the longest suffix has 7 tokens
    "batch_prefix": (lambda m, d: m.generate_batch(PREFIXED, NEW, stop_token=3, decoder=d, shared_prefix=True),
                     dict(batch_size=3, per_row=True, shared_prompt=True, max_new=7 + NEW)),
    "queue": (lambda m, d: m.generate_batch(QUEUE, NEW, stop_token=3, decoder=d, batch_size=2),
              dict(batch_size=2, per_row=True)),
    "queue_shared": (lambda m, d: m.generate_batch([PROMPT] * 5, [6, 2, 5, 3, 6], decoder=d, batch_size=3,
                                                   shared_prompt=True),
                     dict(batch_size=3, per_row=True, shared_prompt=True, max_new=NEW)),
}


@pytest.fixture
def decoders(monkeypatch):
    """Every Decoder constructed and every Decoder released while the test runs."""
    made, released = [], []
    init, release = Decoder.__init__, Decoder.release
    monkeypatch.setattr(Decoder, "__init__", lambda self, *a, **k: (made.append(self), init(self, *a, **k))[1])
    monkeypatch.setattr(Decoder, "release", lambda self: (released.append(self), release(self))[1])
    return made, released


def _lists(y):
    return y.tolist() if torch.is_tensor(y) else [t.tolist() for t in y]


def _shadows(m):
    return [getattr(p, "compute", None) for p in m.parameters()]


@pytest.mark.parametrize("path", list(PATHS))
def test_a_decoder_that_fits_is_used_and_not_released(model, decoders, path):
    call, fit = PATHS[path]
    made, released = decoders
    torch.manual_seed(7)
    want = _lists(call(model, None))
    assert len(made) == 1 and released == made  # the temporary one
    assert all(s is None for s in _shadows(model))
    del made[:], released[:]
    torch.manual_seed(7)  # the same draws in the same order: the decoder's salt, the call's, the samples
    dec = Decoder(model, use_graph=False, **fit)
    got = _lists(call(model, dec))
    assert made == [dec] and not released
    assert all(s is not None for s in _shadows(model))
    assert got == want
    assert len({tuple(y) for y in got}) > 1  # sampled, not greedy: the order of the draws shows
    dec.release()
    assert all(s is None for s in _shadows(model))


MISFITS = {  # misfit -> (a path, the arguments of a decoder that does not fit it)
    "B": ("batch", dict(batch_size=2, per_row=True)),
    "B_queue": ("queue", dict(batch_size=3, per_row=True)),
    "per_row": ("batch", dict(batch_size=3)),
    "per_row_cached": ("cached", dict(batch_size=4, per_row=True)),
    "quantize": ("batch", dict(batch_size=3, per_row=True, quantize="int8")),
    "kv_quantize": ("batch", dict(batch_size=3, per_row=True, kv_quantize="int8")),
    "kv_quantize_cached": ("cached", dict(batch_size=4, kv_quantize="int8")),
    "shared_for_unshared": ("batch", dict(batch_size=3, per_row=True, shared_prompt=True, max_new=NEW)),
    "unshared_for_shared": ("batch_shared", dict(batch_size=3, per_row=True)),
    "unshared_for_shared_cached": ("cached_shared", dict(batch_size=4)),
    "unshared_for_prefix": ("batch_prefix", dict(batch_size=3, per_row=True)),
    "unshared_for_shared_queue": ("queue_shared", dict(batch_size=3, per_row=True)),
    "R_shared": ("batch_shared", dict(batch_size=3, per_row=True, shared_prompt=True, max_new=NEW - 1)),
    "R_cached": ("cached_shared", dict(batch_size=4, shared_prompt=True, max_new=NEW - 1)),
    "R_prefix": ("batch_prefix", dict(batch_size=3, per_row=True, shared_prompt=True, max_new=7 + NEW - 1)),
    "R_queue": ("queue_shared", dict(batch_size=3, per_row=True, shared_prompt=True, max_new=NEW - 1)),
}


@pytest.mark.parametrize("misfit", list(MISFITS))
def test_a_decoder_that_does_not_fit_is_neither_used_nor_released(model, decoders, misfit):
    path, args = MISFITS[misfit]
    call, fit = PATHS[path]
    made, released = decoders
    dec = Decoder(model, use_graph=False, **args)
    dec.pos.fill_(3)  # a state a prefill or a step would overwrite
    dec.gen.copy_(torch.arange(dec.gen.numel()).view_as(dec.gen))
    pos, gen, shadows = dec.pos.clone(), dec.gen.clone(), _shadows(model)
    assert all(s is not None for s in shadows)
    del made[:]
    ys = call(model, dec)
    assert len(ys) == fit["batch_size"] or path.startswith("queue")
    assert len(made) == 1 and made[0] is not dec and released == made
    built = made[0]
    assert (built.B, built.per_row, built.quantize, built.kv_quantize, built.shared) == (
        fit["batch_size"], fit.get("per_row", False), None, None, fit.get("shared_prompt", False))
    assert not built.shared or built.R == fit["max_new"]
    assert torch.equal(dec.pos, pos) and torch.equal(dec.gen, gen)
    assert all(a is b for a, b in zip(_shadows(model), shadows))
    dec.release()
    assert all(s is None for s in _shadows(model))


@pytest.mark.parametrize("flags, rounds, sizes", [
    (["--sample_batch=3", "--num_samples=6"], 2, [3]),
    (["--sample_batch=3", "--num_samples=7"], 3, [3, 1]),
    (["--sample_batch=3", "--num_samples=7", "--shared_prompt=True"], 3, [3, 1]),
    (["--sample_batch=3", "--num_samples=6", "--shared_prefix=True"], 2, [3]),  # equal prompts: all but one token
    (["PROMPTS", "--num_samples=3", "--shared_prefix=True"], 3, [3]),
    (["PROMPTS", "--num_samples=2", "--stop_token=5"], 2, [3]),
    (["--num_samples=3"], 3, [1]),
])
def test_sample_keeps_decoders_that_its_calls_accept(model, decoders, tmp_path, monkeypatch, flags, rounds, sizes):
    """One construction per batch size in a whole run: every round's call took the kept decoder."""
    made, released = decoders
    (tmp_path / "prompt.txt").write_text("1,2,3")
    (tmp_path / "prompts.txt").write_text("9,8,7,1,2,3\n9,8,7,4,5\n9,8,7,6\n")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    torch.save({"model": model.state_dict(), "model_args": ARGS, "iter_num": 0, "best_val_loss": 0.0, "config": {}},
               tmp_path / "ckpt.pt")
    flags = [f"--prompts_file={tmp_path / 'prompts.txt'}" if f == "PROMPTS" else f for f in flags]
    calls = []
    real = Decoder.reseed
    monkeypatch.setattr(Decoder, "reseed", lambda self: (calls.append(self), real(self))[1])
    outs = sample.main([f"--out_dir={tmp_path}", "--device=cpu", f"--max_new_tokens={NEW}", "--top_k=20",
                        f"--start=FILE:{tmp_path / 'prompt.txt'}"] + flags)
    assert [d.B for d in made] == sizes
    # one call per round, each on a kept decoder
    assert len(calls) == rounds and all(any(d is k for k in made) for d in calls)
    assert sorted(map(id, released)) == sorted(map(id, made))  # sample.py released them itself, once each
    assert len(outs) == sum(int(f.split("=")[1]) for f in flags if f.startswith("--num_samples")) * (
        3 if any("prompts_file" in f for f in flags) else 1)
