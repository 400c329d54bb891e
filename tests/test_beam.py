"""Beam search off the GPU: the rule (``ops.beam_select``) on hand-made inputs, ``generate_beam`` against a
search written out as a recompute loop, and the refusals."""

import pytest
import torch

from nanosandbox_amd import ops
from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime import decode
from test_decode_plumbing import ARGS, PROMPT

INF = float("inf")
NEW = 6

# name -> (scores, done, top_ids, top_lp, stop_token), (parent, token, scores, done)
RULE = {
    # three candidates worth -1: (parent ascending, j ascending) keeps (0, 0) and (0, 1)
    "ties": (([0.0, 0.0], [0, 0], [[5, 6], [7, 8]], [[-1.0, -1.0], [-1.0, -2.0]], None),
             ([0, 0], [5, 6], [-1.0, -1.0], [0, 0])),
    # beam 1 is finished: one candidate, worth its score, with the stop token; beam 0's second id is the stop token
    "finished": (([-1.0, -1.0, -2.0], [0, 1, 0], [[11, 9, 13], [1, 2, 3], [21, 22, 23]],
                  [[-0.5, -0.5, -3.0], [0.0, 0.0, 0.0], [0.0, -1.0, -2.0]], 9),
                 ([1, 0, 0], [9, 11, 9], [-1.0, -1.5, -1.5], [1, 0, 1])),
    # the start state: W copies of one distribution, only beam 0 counts
    "start": (([0.0, -INF, -INF], [0, 0, 0], [[4, 2, 7]] * 3, [[-0.125, -2.0, -3.0]] * 3, 2),
              ([0, 0, 0], [4, 2, 7], [-0.125, -2.0, -3.0], [0, 1, 0])),
    # -inf is a value: among three of them the order is the candidates' own
    "minus_inf": (([0.0, -INF], [0, 0], [[5, 6], [7, 8]], [[-1.0, -INF], [-1.0, -2.0]], None),
                  ([0, 0], [5, 6], [-1.0, -INF], [0, 0])),
    # no stop token: a finished beam is fed id 0 and nothing else finishes
    "no_stop": (([-1.0, -2.0], [1, 0], [[1, 2], [3, 4]], [[-0.25, -0.5], [-0.5, -0.75]], None),
                ([0, 1], [0, 3], [-1.0, -2.5], [1, 0])),
}


@pytest.mark.parametrize("name", list(RULE))
def test_beam_select_rule(name):
    (scores, done, ids, lp, stop), (parent, token, new, fin) = RULE[name]
    got = ops.beam_select(torch.tensor(scores), torch.tensor(done, dtype=torch.bool),
                          torch.tensor(ids, dtype=torch.int32), torch.tensor(lp), stop)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.int64 and got[2].dtype == torch.float32
    assert [t.tolist() for t in got] == [parent, token, new, [bool(f) for f in fin]]


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return GPT(GPTConfig(**ARGS)).eval()


def search(model, prompt, new, W, stop=None):
    """Beam search as a recompute loop: no cache, no decoder -> (new tokens per hypothesis, scores)."""
    hyps, scores, done = [[] for _ in range(W)], torch.tensor([0.0] + [-INF] * (W - 1)), torch.zeros(W, dtype=torch.bool)
    for _ in range(new):
        logits = torch.stack([model.forward_logits(torch.tensor(prompt.tolist() + h)[None])[0, -1] for h in hyps])
        rec = ops.token_logprobs(logits.float(), torch.zeros(W, dtype=torch.int64), top=W)
        parent, token, scores, now = ops.beam_select(scores, done, rec.top_ids, rec.top, stop)
        hyps = [hyps[p] + ([] if done[p] else [t]) for p, t in zip(parent.tolist(), token.tolist())]
        done = now
    return hyps, scores


@pytest.mark.parametrize("stop", [False, True], ids=["no-stop", "stop"])
@pytest.mark.parametrize("W", [2, 3, 8])
def test_generate_beam_is_the_recompute_search(model, W, stop):
    with torch.no_grad():
        want, scores = search(model, PROMPT, NEW, W)
        if stop:  # the best hypothesis's third token: it finishes early
            stop = want[0][2]
            want, scores = search(model, PROMPT, NEW, W, stop)
            assert any(len(h) < NEW and h[-1] == stop for h in want)
        outs, got = model.generate_beam(PROMPT, NEW, W, stop_token=stop if stop else None)
    assert [o.tolist() for o in outs] == [PROMPT.tolist() + h for h in want]
    assert torch.allclose(got, scores, rtol=0, atol=1e-5)


def test_one_beam_is_greedy_decoding(model):
    outs, score = model.generate_beam(PROMPT, NEW, 1)
    want = model.generate_cached(PROMPT[None], NEW, top_k=1)
    assert len(outs) == 1 and outs[0].tolist() == want[0].tolist() and score.shape == (1,)
    assert abs(float(score) - float(model.score(want).token[0, PROMPT.numel() - 1:].sum())) < 1e-4


REFUSALS = [
    (dict(num_beams=0), "num_beams must be an int in 1 .. 8"),
    (dict(num_beams=9), "num_beams must be an int in 1 .. 8"),
    (dict(num_beams=2, kv_quantize="int8"), "beam search reads its hypotheses' keys through the bf16 row caches"),
    (dict(num_beams=2, speculate=2), "beam search cannot be combined with speculate"),
    (dict(num_beams=2, max_new_tokens=ARGS["block_size"]), "beam search needs the KV-cache path"),
    (dict(num_beams=2, idx=PROMPT[None].repeat(2, 1)), "beam search takes one prompt per call"),
    (dict(num_beams=2, temperature=0.8, top_k=5), "beam search does not sample: it takes no temperature, top_k"),
]


@pytest.mark.parametrize("kw, message", REFUSALS)
def test_refusals(model, kw, message):
    call = {"idx": PROMPT, "max_new_tokens": NEW, **kw}
    with pytest.raises(ValueError, match=message):
        model.generate_beam(**call)


def test_more_beams_than_ids_are_refused():
    tiny = GPT(GPTConfig(**{**ARGS, "vocab_size": 5})).eval()
    with pytest.raises(ValueError, match="exceeds the vocabulary"):
        tiny.generate_beam(torch.tensor([1, 2]), NEW, 6)
    assert decode.graph_key(decode.Sampling(stop_token=3), beams=4) == (1.0, None, "beam", 4, 3)


def test_sample_cli_prints_ranked_hypotheses(model, tmp_path, monkeypatch, capsys):
    from nanosandbox_amd import sample

    torch.save({"model": model.state_dict(), "model_args": ARGS, "iter_num": 0, "best_val_loss": 0.0, "config": {}},
               tmp_path / "ckpt.pt")
    (tmp_path / "prompts.txt").write_text("5,9,2,44\n12,3,77,5,20\n")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    outs = sample.main([f"--out_dir={tmp_path}", "--device=cpu", f"--max_new_tokens={NEW}", "--num_beams=4",
                        f"--prompts_file={tmp_path / 'prompts.txt'}"])
    scores = [float(ln.split()[1]) for ln in capsys.readouterr().out.splitlines() if ln.startswith("logprob")]
    assert len(outs) == 8 and len(set(outs)) == 8 and scores[:4] == sorted(scores[:4], reverse=True)
    want, _ = model.generate_beam(torch.tensor([5, 9, 2, 44]), NEW, 4)
    assert outs[:4] == [",".join(map(str, y.tolist())) for y in want]
