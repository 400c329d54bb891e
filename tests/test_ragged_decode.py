"""Batched generation of unequal-length prompts with a stop token (runtime/decode.py,
``Decoder(per_row=True)`` / ``GPT.generate_batch``) on the CPU: the fp32 torch paths of the
per-row decode ops against the full-recompute model."""

import pytest
import torch

from nanosandbox_amd.models import GPT, GPTConfig
from nanosandbox_amd.runtime.decode import Decoder

LENS = (3, 7, 12)
V = 97


def _model():
    torch.manual_seed(0)
    return GPT(GPTConfig(block_size=48, vocab_size=V, n_layer=2, n_head=4, n_embd=64, dropout=0.0,
                         bias=True)).eval()


def _prompts():
    g = torch.Generator().manual_seed(5)
    return [torch.randint(0, V, (n,), generator=g) for n in LENS]


@pytest.fixture(scope="module")
def greedy():
    """The reference: every prompt on its own through the recompute loop, 20 greedy tokens,
    with the smallest top-1 / top-2 logit gap met on the way."""
    m, prompts = _model(), _prompts()
    refs, gaps = [], []
    with torch.no_grad():
        for p in prompts:
            y = m.generate(p[None], 20, top_k=1)[0]
            top2 = torch.topk(m.forward_logits(y[None, :-1])[0, p.numel() - 1:], 2, dim=-1).values
            refs.append(y)
            gaps.append(float((top2[:, 0] - top2[:, 1]).min()))
    return m, prompts, refs, gaps


def test_teacher_forced_ragged_logits_match_full_forward():
    m = _model()
    steps = 12
    g = torch.Generator().manual_seed(7)
    seqs = [torch.randint(0, V, (n + steps,), generator=g) for n in LENS]
    idx = torch.zeros(3, max(LENS), dtype=torch.int64)
    for b, n in enumerate(LENS):
        idx[b, :n] = seqs[b][:n]
        idx[b, n:] = (b + 11) % V  # right padding: any valid id
    with torch.no_grad():
        full = [m.forward_logits(s[None])[0] for s in seqs]  # each row's own unpadded sequence
        dec = Decoder(m, 3, use_graph=False, per_row=True)
        lg = dec.prefill(idx, torch.tensor(LENS))
        for b, n in enumerate(LENS):
            assert torch.allclose(lg[b], full[b][n - 1], atol=1e-4, rtol=1e-4), b
        for t in range(steps):
            lg = dec.step(torch.stack([seqs[b][n + t] for b, n in enumerate(LENS)]))
            for b, n in enumerate(LENS):
                assert torch.allclose(lg[b], full[b][n + t], atol=1e-4, rtol=1e-4), (b, t)
    assert dec.positions == [15, 19, 24]


def test_generate_batch_greedy_matches_recompute(greedy):
    m, prompts, refs, gaps = greedy
    # the comparison is only meaningful where the argmax is stable under the 1e-4 logit tolerance
    assert min(gaps) >= 1e-3, gaps
    outs = m.generate_batch(prompts, 20, top_k=1)
    assert len(outs) == 3
    for o, r in zip(outs, refs):
        assert torch.equal(o, r)


def test_generate_batch_stop_token(greedy):
    m, prompts, refs, _ = greedy
    stop = 28
    new = [r[n:].tolist() for r, n in zip(refs, LENS)]
    # the inputs: the length-7 row draws 28 as its 4th token, the others never do
    assert new[1][:4] == [92, 92, 92, 28] and stop not in new[0] and stop not in new[2]
    outs = m.generate_batch(prompts, 20, top_k=1, stop_token=stop)
    n_new = [o.numel() - n for o, n in zip(outs, LENS)]
    assert any(2 <= k < 20 for k in n_new) and any(k == 20 for k in n_new)
    assert n_new[1] == 4 and int(outs[1][-1]) == stop and torch.equal(outs[1], refs[1][:7 + 4])
    assert torch.equal(outs[0], refs[0]) and torch.equal(outs[2], refs[2])


def test_generate_batch_row_past_block_size_goes_alone(greedy):
    """A row that cannot live in the cache is generated on its own; the others share the batch."""
    m, prompts, refs, _ = greedy
    torch.manual_seed(3)
    long = torch.randint(0, V, (40,))
    ref = m.generate(long[None], 20, top_k=1)[0]
    outs = m.generate_batch([prompts[0], long, prompts[2]], 20, top_k=1)
    assert torch.equal(outs[1], ref) and torch.equal(outs[0], refs[0]) and torch.equal(outs[2], refs[2])


def test_sample_cli_batches(tmp_path, monkeypatch):
    from nanosandbox_amd import sample

    m = _model()
    ck = {"model": m.state_dict(), "model_args": dict(block_size=48, vocab_size=V, n_layer=2, n_head=4, n_embd=64,
                                                      bias=True, dropout=0.0),
          "iter_num": 0, "best_val_loss": 0.0, "config": {}}
    torch.save(ck, tmp_path / "ckpt.pt")
    (tmp_path / "prompt.txt").write_text("1,2,3")
    (tmp_path / "prompts.txt").write_text("1,2,3\n9,8,7,6,5,4,3\n")
    monkeypatch.setattr(sample, "_codec", lambda ck, dd: ((lambda s: [int(t) for t in s.split(",")]),
                                                          (lambda ids: ",".join(map(str, ids)))))
    base = [f"--out_dir={tmp_path}", "--device=cpu", "--max_new_tokens=6", "--top_k=1"]
    start = f"--start=FILE:{tmp_path / 'prompt.txt'}"
    one = sample.main(base + [start, "--num_samples=1"])
    outs = sample.main(base + [start, "--num_samples=3", "--sample_batch=3"])
    assert len(outs) == 3 and all(o == one[0] for o in outs)
    rag = sample.main(base + ["--num_samples=1", f"--prompts_file={tmp_path / 'prompts.txt'}"])
    assert len(rag) == 2
    assert rag[0].startswith("1,2,3,") and rag[1].startswith("9,8,7,6,5,4,3,")
    assert [len(t.split(",")) for t in rag] == [9, 13]
    assert rag[0] == one[0]  # the short prompt is not disturbed by its longer neighbour
    # a stop token ends the printed text before it
    first = int(one[0].split(",")[3])
    cut = sample.main(base + [start, "--num_samples=1", f"--stop_token={first}"])
    assert cut == ["1,2,3"]
