"""Incremental decoding with per-layer KV caches, one token's forward replayed as a HIP graph.

nanoGPT's ``generate`` (reference ``sample.py`` -> ``model.generate``, SURVEY.md §2.3
U-M11/U-S1) runs the whole context through the model for every new token: O(T)
work per token for the projections and O(T^2) for attention, and at serving batch
sizes a few hundred tiny kernel launches per token whose host overhead dominates.

``Decoder`` keeps K and V of every layer in bf16 caches [B, H, block_size, D]
(``ops.kv_append``) and decodes one position at a time:

* ``prefill(idx)``: the prompt goes through the normal fused forward (flash
  attention over the prompt), each layer's K/V rows are written to the caches, and
  the last position's logits are returned;
* ``step(tok)``: embedding of the new token at position ``pos`` -> per layer
  residual-add+LN+c_attn -> append K/V + single-query attention over the cache
  (``ops.decode_attention``: split-K flash-decoding kernels) -> combine+c_proj ->
  residual-add+LN+c_fc+GELU -> c_proj -> ... -> residual-add+ln_f+lm_head (at batch
  1 each arrow's producer runs in the prologue of the next weight-streaming kernel).  ``pos`` lives in a device tensor
  that the step itself increments, so on the GPU the whole step is captured once
  as a ``torch.cuda.CUDAGraph`` and replayed per token (one launch per token).

Sampling (temperature, top-k, multinomial) is nanoGPT's distribution, drawn on the
device by one kernel (``ops.sample_topk_``: radix-select threshold, softmax mass, scan,
counter-hash uniform) that writes the id straight into the fed-token buffer and into
``gen`` at the device position.  ``run(n)`` captures step + sampling as one graph, so
n tokens are n replays with no host round trip.  ``top_p`` (nucleus) and ``min_p``
narrow the kept set inside the same kernel launch (``ops.filter_logits`` states the
rule); a captured graph is keyed by them only when one of them is on.
``Decoder(..., per_row=True)`` keeps one position and one finished flag per sequence
(``pos`` and ``done``, int64 [B] on the device): prompts of unequal lengths share a
batch (``prefill(idx, lengths)`` on a right-padded ``idx``), the attention and sampling
kernels read ``pos[b]``, and a row that draws the stop token is frozen inside the
captured step: its position stops, it is fed the same token again (rewriting the same
cache row with the same values) and it draws nothing.  ``generate_batch`` is the
list-of-prompts front end.
``Decoder(..., quantize="int8")`` decodes the model whose linear weights (c_attn, both
c_proj, c_fc and the tied lm_head / wte) are the per-row int8 quantization of the
model's (``ops.quantize_rows_int8``): every step streams int8 weights through the
``_q8`` forms of the same kernels (half the bytes, the same launches, the same captured
graph), and prefill and the embedding read the dequantized weights through the
``compute`` shadows, so prompt and steps see one model.
``Decoder(..., kv_quantize="int8")`` keeps the caches as int8 rows with one fp32 scale per
row (``ops.QuantCache``: 68 bytes per K or V row instead of 128, so a step reads 0.53x the
cache bytes and the caches take 0.53x the memory).  The prompt goes through flash attention
on its own unquantized K / V as always and its rows are then stored quantized
(``ops.quantize_cache_rows``); every step quantizes the new token's K / V rows, appends them
and attends over the dequantized rows 0 .. pos, its own included, so a step is a function of
the cache contents.  Unlike the int8-weight mode, prompt and steps therefore do not see one
model: the prompt's own attention is unquantized, the usual practice for KV quantization.
Any batch size, per_row or not, with or without ``quantize="int8"``; same launches, same
captured graph (the ``_kv8`` forms of the append and attention kernels).
``Decoder(..., shared_prompt=True, max_new=R)`` is for many samples of one prompt
(``sample.py --sample_batch=N``, ``generate_batch([p] * N, ..., shared_prompt=True)``): the
prompt runs through the model once, as one row (``prefill_shared``), into prompt caches
[1, H, block_size, D] that the whole batch attends over, and every row caches only the
tokens it generates, [B, H, R, D] (R = ``max_new`` or block_size), the token at absolute
position p in slot p - ``plen``.  A step's attention (``ops.decode_attention_shared``) reads
the prompt's K / V once per head for all rows, P + B n cache rows where the unshared form
reads B (P + n); the prompt length lives on the device (``plen``), so one captured graph
serves every prompt, and the rest of the step (embedding at the absolute position,
linears, sampler, position advance, stop tokens) is the unshared one.  The prompt's ids and
logits are kept, so a second round of samples of the same prompt does not encode it again
(``prefills`` counts the real ones).  At least 2 rows, per_row or not, with or without
``quantize="int8"``, not with ``kv_quantize``; on the GPU bf16 and head_dim 64 only.
Prompts that share only a prefix (a system prompt followed by different questions;
``generate_batch(..., shared_prefix=True)``, ``sample.py --shared_prefix=True``) use the same
decoder, per_row: ``prefill_shared(prefix)`` caches the prefix once, and
``prefill_suffixes(idx, lengths)`` runs every row's right-padded suffix through the model at
positions P .., its K / V rows into row-cache slots 0 .. S - 1 and its queries over the prompt
cache plus the row's own earlier suffix keys (``ops.prefix_attention``: one attention kernel
that reads the prefix cache where it lies, so nothing is materialised per row and no prefix
query is computed again).  ``pos`` becomes P + lengths and the steps are the shared-prompt
ones, unchanged: a row's slots hold suffix and generated tokens alike (slot = position - P).
A queue of prompts longer than the batch (``generate_batch(..., batch_size=B)`` or one budget
per prompt, ``sample.py --serve_batch=B``) is served through B rows of a per_row decoder whose
finished rows are refilled (``Decoder.serve``).  Three per-row things make a row reusable: its
token budget is on the device (``end``: the position of the request's last token; the sampler
finishes the row there as it does at the stop token), its sampling stream is keyed by the
request (``key``), not the row, and ``admit(rows, idx, lengths)`` prefills new prompts into a
chosen subset of rows of the running caches (``ops.kv_append(rows=)``: one launch per layer)
without touching any other row; on a shared_prompt decoder an admission only puts the row back
to the prompt's end.  The loop replays the captured step ``DONE_POLL`` times (``run(...,
queue=True)``: the same step with the keyed sampler, a graph of its own), reads ``done`` and
``pos`` back once, harvests the finished rows, admits the next prompts into all freed rows in
one pass and draws their first tokens alone (``sample_admitted``); no step waits for the host.
``Decoder(..., speculate=K, spec_ngram=N)`` (1 <= K <= 7; implies per_row) verifies K drafted tokens
per captured step.  A step feeds every row's token and K guessed continuations (``stok`` at the
positions ``spos``, int64 [B, K + 1] on the device) as B (K + 1) rows through the same embedding and
linear ops, attends with ``ops.decode_attention_spec`` (K + 1 consecutive queries of one sequence
against one cache, bit for bit the K + 1 successive single-query calls), draws the token of every
fed position with the stream the plain per-row decoder uses for it (the sampler's uniform is a
counter hash of (salt, row, position): the ``row_key`` form over B (K + 1) rows, row (b, j) keyed
(b, pos[b] + j + 1), into scratch) and ``ops.spec_accept_`` keeps a draft if and only if it equals
that draw.  For a deterministic draft this accepts with probability p(draft), as rejection sampling
does, and what is emitted is always the model's own draw: the tokens are the plain decoder's for
any temperature / top-k / top-p / min-p, with no second sampler and no residual distribution.
Drafts are n-gram lookup in the row's own history ``gen[b, 0 .. pos[b]]`` (``ops.ngram_draft``, in the
accept kernel's launch; ``prefill`` therefore also copies the prompt ids into ``gen``), or come from
a table (``set_draft_table``: for measuring a step at a chosen acceptance).  A row advances by what
it accepts inside the captured graph: there is no ``advance_pos_`` and no ``pos_inc`` in such a
step, ``run(n)`` gives every row a budget on the device (``end``), the graph key gains ``("spec", K,
N)``, the loop looks at ``done`` every ``DONE_POLL`` replays (sooner when no row can need that many)
and ``spec_stats`` reads the per-row counters back.  With ``quantize="int8"``, ``stop_token``,
``top_p`` / ``min_p`` and eager mode; ``kv_quantize``, ``shared_prompt`` / ``shared_prefix``, the queue, on
the GPU B (K + 1) > 16 and a model without the fused decode kernels raise ValueError.  Rows near the
end of the cache have dead queries (positions >= block_size): they store nothing, come out as
zeros and are never accepted.  With ``speculate`` unset nothing of this exists: every launch,
graph key and result is what it was.
``Decoder(..., penalize=True)`` is the mode for repetition, presence and frequency penalties
(``ops.penalize_logits`` states the rule).  Such a decoder owns the count table ``cnt`` (int32 [B, V
rounded up to 4]): ``cnt[b, v]`` is how often id v occurs in row b's text, its prompt without the
padding (prefix plus suffix on a shared-prefix decoder) and every token drawn for it.  Every
prefill form and ``admit`` rebuild the rows they start (``ops.token_counts_``: one launch; a
shared_prompt decoder keeps its prompt's histogram as ``cnt0`` and copies it), and every draw goes
through the penalised sampler (``ops.sample_topk_(counts=)``), which applies the penalties as it
loads a row and counts the id it draws: the step keeps its launches, and with no penalty passed
the parameters are the identity, so ``cnt`` never goes stale.  The graph key gains ``("pen", rp, pp,
fp)``.  With per_row, ``stop_token``, ``top_p`` / ``min_p``, both quantizations, ``shared_prompt`` /
``shared_prefix``, the queue and eager mode; ``speculate`` raises ValueError (a verified position's
counts would have to include the drafts before it).  Without ``penalize`` there is no table
(``cnt`` is None) and every launch, graph key and result is what it was.
``Decoder(..., logprobs=N)`` (0 .. 8; None: off) records how likely the model found every token it
drew: ``lp[b, p]`` (fp32 [B, block_size + 1], indexed like ``gen``) is the log-probability of ``gen[b, p]``
under the raw logits the sampler was handed, before penalties, temperature and filters: the model's
own distribution, the quantity ``GPT.score`` returns for a given text (``ops.token_logprobs`` states
the rule), and with N > 0 ``top_ids[b, p, :]`` / ``top_lp[b, p, :]`` hold the N most likely ids there and
their log-probabilities.  One more launch per draw, right after the sampler inside ``sample_into``
(``ops.token_logprobs_step_``), so the prefill's first token, the eager step and every captured graph
record alike, and ``sample_admitted`` does the same.  ``lp_last`` (int64 [B]) is the position every row
recorded last; a row whose position has not moved since (it was finished before this sampler call)
records nothing, a row that finishes in this call still records its last token, and every prefill
form and ``admit`` put the rows they start back to -1.  The graph key gains ``("lp", N)``.  With
per_row, ``stop_token``, ``top_p`` / ``min_p``, the penalties, both quantizations, ``shared_prompt`` /
``shared_prefix``, the queue and eager mode; ``speculate`` raises ValueError (a verified position can
be written by more than one step).  Without ``logprobs`` there are no buffers (``lp`` is None) and
every launch, graph key and result is what it was.
The caches hold at most ``block_size`` positions; ``GPT.generate_cached`` falls
back to the recompute loop when prompt + new tokens exceed that (nanoGPT crops the
context there, which a cache cannot do without re-encoding).
"""

from __future__ import annotations

import contextlib
from typing import NamedTuple

import torch

from .. import ops


class Sampling(NamedTuple):
    """The sampling settings of a call, normalised once (``sampling``): what is off is None."""
    temperature: float = 1.0
    top_k: int | None = None
    stop_token: int | None = None
    top_p: float | None = None
    min_p: float | None = None
    penalties: tuple | None = None  # (repetition_penalty, presence_penalty, frequency_penalty) as floats


def sampling(temperature=1.0, top_k=None, stop_token=None, top_p=None, min_p=None, repetition_penalty=None,
             presence_penalty=None, frequency_penalty=None) -> Sampling:
    """The ``Sampling`` of a call's raw arguments, validated (``ops.check_sampling_filters``,
    ``ops.check_sampling_penalties``: ValueError): a stop token < 0 means none, a filter that is off
    (``top_p`` >= 1, ``min_p`` 0) and penalties that are all off (1, 0 and 0, or None) are None.
    ``top_k`` stays as given (None or 0: off).  A ``Sampling`` in ``temperature``'s place is the
    value itself, whatever follows it: the public entry points build it once and hand it on so."""
    if isinstance(temperature, Sampling):
        return temperature
    ops.check_sampling_filters(top_p, min_p)
    ops.check_sampling_penalties(repetition_penalty, presence_penalty, frequency_penalty)
    pen = (1.0 if repetition_penalty is None else float(repetition_penalty),
           0.0 if presence_penalty is None else float(presence_penalty),
           0.0 if frequency_penalty is None else float(frequency_penalty))
    return Sampling(temperature, top_k, None if stop_token is None or stop_token < 0 else stop_token,
                    None if top_p is None or float(top_p) >= 1.0 else float(top_p),
                    None if min_p is None or float(min_p) <= 0.0 else float(min_p),
                    None if pen == (1.0, 0.0, 0.0) else pen)


def sampling_filters(top_p=None, min_p=None):
    """Validated (top_p, min_p) with a filter that is off (``top_p`` >= 1, ``min_p`` 0) as None."""
    return sampling(top_p=top_p, min_p=min_p)[3:5]


def sampling_penalties(repetition_penalty=None, presence_penalty=None, frequency_penalty=None):
    """Validated (repetition_penalty, presence_penalty, frequency_penalty) as floats, or None when
    all three are off (1, 0 and 0, or None)."""
    return sampling(repetition_penalty=repetition_penalty, presence_penalty=presence_penalty,
                    frequency_penalty=frequency_penalty).penalties


def graph_key(smp: Sampling, per_row=False, queue=False, spec=None, table=False, penalize=False,
              logprobs=None) -> tuple:
    """The key of a captured sampling step in ``Decoder.sgraphs``: (temperature, top_k), then the stop
    token (a ``per_row`` decoder: None included), (top_p, min_p) if either is on (without them: the
    keys of the top-k sampler), ``"queue"``, ``("spec", K, N)`` (``spec`` = (K, N)) and ``"table"`` (a
    draft table is set), ``("pen", rp, pp, fp)`` on a penalising decoder (the identity (1, 0, 0) when
    the call passes none) and ``("lp", N)`` on one that records log-probabilities."""
    key = (float(smp.temperature), smp.top_k) + ((smp.stop_token,) if per_row else ())
    if smp.top_p is not None or smp.min_p is not None:
        key += (smp.top_p, smp.min_p)
    if queue:
        key += ("queue",)
    if spec:
        key += ("spec", *spec) + (("table",) if table else ())
    if penalize:
        key += ("pen", *(smp.penalties or (1.0, 0.0, 0.0)))
    if logprobs is not None:
        key += ("lp", logprobs)
    return key


def _check(quantize=None, kv_quantize=None, shared_prompt=False, shared_prefix=False, queue=False, speculate=None,
           spec_ngram=3, penalize=False, logprobs=None, rows=None, max_new=None):
    """Every rule on a mode that depends on neither the model nor the device, for ``Decoder`` and the
    front ends alike: ValueError for what does not compose, never a silent plain step -> (K, N,
    logprobs), the drafted tokens and n-gram length of a speculative call (K = 0: none) and
    ``logprobs`` validated (None: off; 0 .. 8 alternatives).  ``penalize``: a count table, or a call
    with a penalty on; ``rows`` / ``max_new``: a decoder's own (a front end plans them afterwards)."""
    if quantize not in (None, "int8"):
        raise ValueError(f"quantize must be None or 'int8', got {quantize!r}")
    if kv_quantize not in (None, "int8"):
        raise ValueError(f"kv_quantize must be None or 'int8', got {kv_quantize!r}")
    if shared_prompt and kv_quantize:
        raise ValueError("shared_prompt keeps bf16 caches: it cannot be combined with kv_quantize")
    if shared_prefix and shared_prompt:
        raise ValueError("shared_prefix and shared_prompt are two forms of sharing: pass one of them")
    if shared_prefix and kv_quantize:
        raise ValueError("shared_prefix keeps bf16 caches: it cannot be combined with kv_quantize")
    logprobs = ops.check_logprobs(logprobs)
    K, N = int(speculate or 0), 3
    if K:
        N = 3 if spec_ngram is None else int(spec_ngram)
        if logprobs is not None:
            raise ValueError("speculate cannot be combined with logprobs: a verified position can be written by more "
                             "than one step")
        if not 1 <= K <= ops.functional.SPEC_MAX_DRAFTS:
            raise ValueError(f"speculate must be in 1 .. {ops.functional.SPEC_MAX_DRAFTS} drafted tokens, "
                             f"got {speculate!r}")
        if N < 1:
            raise ValueError(f"spec_ngram must be at least 1, got {spec_ngram!r}")
        if kv_quantize:
            raise ValueError("speculate keeps bf16 caches: it cannot be combined with kv_quantize")
        if shared_prompt or shared_prefix:
            raise ValueError("speculate decodes every row against its own cache: it cannot be combined with "
                             "shared_prompt / shared_prefix")
        if queue:
            raise ValueError("speculative batches are not served as a queue: drop batch_size / per-prompt budgets")
        if penalize:
            raise ValueError("speculate cannot be combined with sampling penalties: a verified position's counts "
                             "would have to include the drafts before it")
    if shared_prompt and rows is not None and rows < 2:
        raise ValueError(f"shared_prompt needs at least 2 rows to share a prompt, got batch size {rows}")
    if max_new is not None and not shared_prompt:
        raise ValueError("max_new sizes the row caches of a shared_prompt decoder")
    return K, N, logprobs


class Decoder:
    def __init__(self, model, batch_size: int, max_len: int | None = None, use_graph: bool | None = None,
                 per_row: bool = False, quantize: str | None = None, kv_quantize: str | None = None,
                 shared_prompt: bool = False, max_new: int | None = None, speculate: int | None = None,
                 spec_ngram: int = 3, penalize: bool = False, logprobs: int | None = None):
        self.K, self.N, logprobs = _check(quantize, kv_quantize, shared_prompt, speculate=speculate,
                                          spec_ngram=spec_ngram, penalize=penalize, logprobs=logprobs,
                                          rows=batch_size, max_new=max_new)
        per_row = per_row or bool(self.K)  # a speculating row advances by its own number of positions
        self.model = model
        self.per_row = per_row
        self.quantize = quantize
        self.kv_quantize = kv_quantize
        self.shared = bool(shared_prompt)
        cfg = model.config
        on_gpu = model.lm_head.weight.is_cuda

        def needs_fused(mode):
            # the shared-prompt attention kernel, the int8-cache kernels and the int8-weight kernels are
            # head_dim-64 bf16 ones, and there is no int8 form of the fallback ops; no silent torch step instead
            if on_gpu and not self.graph_capable(model):
                raise ValueError(f"{mode} needs the fused decode kernels on the GPU: head_dim 64, "
                                 "bfloat16 compute and a vocabulary of at most 53248")
        if shared_prompt:
            needs_fused("shared_prompt")
        if kv_quantize:
            needs_fused("kv_quantize='int8'")
        if self.K:
            needs_fused("speculate")
            # a step runs B * (K + 1) rows through the linears: the skinny kernels' range, no larger GEMM instead
            if on_gpu and batch_size * (self.K + 1) > ops.functional.SKINNY_MAX_ROWS:
                raise ValueError(f"speculate={self.K} decodes at most {ops.functional.SKINNY_MAX_ROWS // (self.K + 1)} "
                                 f"rows on the GPU ({ops.functional.SKINNY_MAX_ROWS} step rows), got batch size "
                                 f"{batch_size}")
        if quantize:
            # the int8 kernels are the single-row and skinny ones; there is no int8 form of the
            # larger-batch GEMMs, and no silent bf16 step instead
            if on_gpu and batch_size > ops.functional.SKINNY_MAX_ROWS:
                raise ValueError(f"quantize='int8' decodes at most {ops.functional.SKINNY_MAX_ROWS} rows on the GPU "
                                 f"(the skinny int8 kernels), got batch size {batch_size}")
            needs_fused("quantize='int8'")
        self.B = batch_size
        self.T = max_len or cfg.block_size
        assert self.T <= cfg.block_size, "caches cannot exceed the position-embedding table"
        self.H = cfg.n_head
        self.D = cfg.n_embd // cfg.n_head
        p = model.lm_head.weight
        self.device = p.device
        self.dtype = model.compute_dtype
        self.rdtype = model.residual_dtype
        shape = (batch_size, self.H, self.T, self.D)
        if kv_quantize:  # int8 rows + one fp32 scale per row (a zero row: bytes 0, scale 1)
            def cache():
                return ops.QuantCache(torch.zeros(shape, device=self.device, dtype=torch.int8),
                                      torch.ones(shape[:3], device=self.device, dtype=torch.float32))
        else:
            def cache():
                return torch.zeros(shape, device=self.device, dtype=self.dtype)
        if shared_prompt:
            # one prompt cache for the batch and, per row, only the tokens it generates itself:
            # the token at absolute position p >= plen lives in row-cache slot p - plen
            self.R = int(max_new) if max_new else self.T
            if not 1 <= self.R <= self.T:
                raise ValueError(f"max_new must be in 1 .. {self.T}, got {max_new}")
            pshape, shape = (1, self.H, self.T, self.D), (batch_size, self.H, self.R, self.D)
            self.pkc = [torch.zeros(pshape, device=self.device, dtype=self.dtype) for _ in range(cfg.n_layer)]
            self.pvc = [torch.zeros(pshape, device=self.device, dtype=self.dtype) for _ in range(cfg.n_layer)]
            self.plen = torch.zeros(1, device=self.device, dtype=torch.int64)
            self.prefills = 0            # prompts actually run through the model
            self._prompt = None          # the cached prompt's token ids ...
            self._prompt_logits = None   # ... and its last position's logits [1, V]
        self.kc = [cache() for _ in range(cfg.n_layer)]
        self.vc = [cache() for _ in range(cfg.n_layer)]
        # position of the token being fed: one for the whole batch, or (per_row) one per sequence
        self.pos = torch.zeros(batch_size if per_row else 1, device=self.device, dtype=torch.int64)
        # per_row: done[b] != 0 once row b has drawn the stop token; such a row is frozen (it is
        # fed the same token at the same position in every later step and draws nothing)
        self.done = torch.zeros(batch_size, device=self.device, dtype=torch.int64) if per_row else None
        self.tok = torch.zeros(batch_size, 1, device=self.device, dtype=torch.int64)
        # generated tokens by position: gen[:, p] is the token fed at position p
        self.gen = torch.zeros(batch_size, self.T + 1, device=self.device, dtype=torch.int64)
        self.salt = int(torch.randint(0, 2 ** 62, (1,)).item())  # sampling stream (torch.manual_seed governs)
        # per-call part of the sampling stream, read by the kernel at run time (so a captured
        # sampling graph, reused across generate calls, draws independent samples each call)
        self.salt_dev = torch.zeros(1, device=self.device, dtype=torch.int64)
        # the serving queue's per-row state (int64 [B] each, allocated when first used): the request a
        # row serves, which keys its sampling stream, and the position of the request's last token
        self.key = None
        self.end = None
        self.queue_stats = {"steps": 0, "admissions": 0, "admitted": 0}
        if self.K:
            # a speculative step's device state: the fed tokens (the row's token and K drafts), their
            # positions and the positions their draws are keyed by (int64 [B, K + 1] each); the draws
            # themselves (ctok, with the sampler's per-position scratch cgen), keyed by the row (rkey);
            # the per-row budget end and the counters (live steps, drafts offered, drafts accepted)
            rows = batch_size * (self.K + 1)
            self.stok, self.spos, self.cpos = (torch.zeros(batch_size, self.K + 1, device=self.device,
                                                           dtype=torch.int64) for _ in range(3))
            self.ctok = torch.zeros(rows, 1, device=self.device, dtype=torch.int64)
            self.cgen = torch.zeros(rows, self.T + 1, device=self.device, dtype=torch.int64)
            self.rkey = torch.arange(batch_size, device=self.device, dtype=torch.int64).repeat_interleave(self.K + 1)
            self.end = torch.full((batch_size,), 2 ** 62, device=self.device, dtype=torch.int64)
            self.spec_counts = torch.zeros(batch_size, 3, device=self.device, dtype=torch.int64)
            self.table = None  # set_draft_table: drafts read from a table instead of the n-gram lookup
        self._admit_logits = None  # [B, V] fp32: the admitted rows' logits at their own row indices
        # penalize: how often every id occurs in a row's text (prompt and drawn tokens), int32 [B, V
        # rounded up to 4] so that the sampler reads it in 16-byte vectors; cnt0 [1, same]: the
        # histogram of a shared_prompt decoder's prompt
        self.cnt = self.cnt0 = None
        if penalize:
            self.cnt = torch.zeros(batch_size, -(-cfg.vocab_size // 4) * 4, device=self.device, dtype=torch.int32)
            if shared_prompt:
                self.cnt0 = torch.zeros(1, self.cnt.shape[1], device=self.device, dtype=torch.int32)
        # logprobs: the drawn tokens' log-probabilities and the N alternatives, indexed like gen, and the
        # position every row recorded last (-1: none yet)
        self.logprobs = logprobs
        self.lp = self.top_ids = self.top_lp = self.lp_last = None
        if logprobs is not None:
            self.lp = torch.full((batch_size, self.T + 1), float("nan"), device=self.device, dtype=torch.float32)
            self.top_ids = torch.full((batch_size, self.T + 1, logprobs), -1, device=self.device, dtype=torch.int32)
            self.top_lp = torch.full((batch_size, self.T + 1, logprobs), float("nan"), device=self.device,
                                     dtype=torch.float32)
            self.lp_last = torch.full((batch_size,), -1, device=self.device, dtype=torch.int64)
        self.use_graph = (self.device.type == "cuda") if use_graph is None else use_graph
        if self.use_graph and not self.graph_capable(model):
            # the fused decode kernels cover head_dim 64, bf16 and V <= 53248; the fallback
            # ops read the position back to the host (pos.item()) or refuse wider vocabs,
            # which a captured graph cannot do: run those configs eagerly
            self.use_graph = False
        self.graph = None      # step(): logits only
        self.sgraphs = {}      # run(): step + sampling + token feedback, per (temperature, top_k[, stop_token])
        self.logits = None
        self.replays = 0
        # compute-dtype weight shadows (``param.compute``, what every op reads): a trained
        # model carries the optimizer's; a freshly loaded one would otherwise convert each
        # fp32 weight on every use (124M: ~750 MB of conversion traffic per token, and
        # inside the captured graph too).  Created here, dropped by ``release()``.
        self._shadowed = []
        self.qweights = {}   # int8 mode: id(parameter) -> ops.QuantWeight
        self._qsaved = []    # (parameter, attribute, had it, value) to put back in release()
        if quantize:
            self._quantize_weights()
        if self.dtype != torch.float32:
            for prm in model.parameters():
                c = getattr(prm, "compute", None)
                if c is None or c.dtype != self.dtype:
                    prm.compute = prm.detach().to(self.dtype)
                    self._shadowed.append(prm)

    @staticmethod
    def graph_capable(model) -> bool:
        cfg = model.config
        return (cfg.n_embd // cfg.n_head == 64 and model.compute_dtype == torch.bfloat16
                and cfg.vocab_size <= 53248)

    def fits(self, batch_size, per_row=False, quantize=None, kv_quantize=None, shared_prompt=False,
             max_new=None, speculate=None, spec_ngram=3, penalize=False, logprobs=None) -> bool:
        """Whether a call that needs ``Decoder(model, batch_size, per_row=..., ...)`` can run on this
        one: the same rows and form, (shared) row caches of at least ``max_new`` slots, and the same
        number of drafted tokens and n-gram length (speculative), and a count table if and only if
        the call penalises, and the log-probability buffers of the call's N alternatives, or none."""
        K = int(speculate or 0)
        return (self.B == batch_size and self.per_row == bool(per_row or K) and self.quantize == quantize
                and self.kv_quantize == kv_quantize and self.shared == bool(shared_prompt)
                and (not self.shared or self.R >= (max_new or self.T))
                and self.K == K and (not K or self.N == int(spec_ngram))
                and (self.cnt is not None) == bool(penalize) and self.logprobs == logprobs)

    def _quantize_weights(self):
        """int8 mode: quantize every linear weight and the tied lm_head / wte table, and point
        their ``compute`` shadows (what prefill and the embedding gather read) at the
        dequantized weights in the compute dtype (fp32 on the CPU included), so the prompt
        runs through the same model as the int8 steps.  Whatever ``compute`` a parameter had
        (a trained model's optimizer shadow) is kept for ``release()``."""
        model = self.model
        params = []
        for block in model.transformer.h:
            params += [block.attn.c_attn.weight, block.attn.c_proj.weight, block.mlp.c_fc.weight,
                       block.mlp.c_proj.weight]
        head = model.lm_head.weight  # tied to wte: the token embeddings are the dequantized rows too
        params.append(head)
        for prm in params:
            qw = ops.quantize_rows_int8(prm)
            self.qweights[id(prm)] = qw
            self._qsaved.append((prm, "compute", hasattr(prm, "compute"), getattr(prm, "compute", None)))
            prm.compute = ops.dequantize(qw).to(self.dtype)
        # the padded lm_head operand of a flat parameter store holds the unquantized weights
        if hasattr(head, "compute_padded"):
            self._qsaved.append((head, "compute_padded", True, head.compute_padded))
            del head.compute_padded
        # copies derived from the earlier shadows (the padded lm_head operand) are stale
        ops.gemm_dispatch.weights_changed()

    def _w(self, prm):
        """The weight a decode op streams: the parameter, or its QuantWeight in int8 mode."""
        return self.qweights.get(id(prm), prm)

    def release(self):
        """Drop the weight shadows this decoder created and its captured graph."""
        for prm in self._shadowed:
            try:
                del prm.compute
            except AttributeError:
                pass
        self._shadowed = []
        for prm, name, had, old in self._qsaved:  # int8 mode: the shadows that were there before
            if had:
                setattr(prm, name, old)
            elif hasattr(prm, name):
                delattr(prm, name)
        if self._qsaved:
            ops.gemm_dispatch.weights_changed()
        self._qsaved = []
        self.qweights = {}
        self.graph = None
        self.sgraphs = {}

    # ------------------------------------------------------------------ layers
    def _prefill_layers(self, x, kc=None, vc=None, prefix=None, rows=None):
        """The prompt x through every block; its K / V rows go to the caches ``kc`` / ``vc``
        (default: the decoder's own; ``prefill_shared`` passes the prompt caches).  ``prefix``
        (``prefill_suffixes``: the prefix length P): x holds the suffixes that follow the cached
        prefix, and every query also attends over prompt-cache rows 0 .. P - 1.  ``rows``
        (``admit``; int64 [n] on the device): row j of x is cache row ``rows[j]``."""
        kc, vc = kc or self.kc, vc or self.vc
        tr = self.model.transformer
        blocks = tr.h
        ln = blocks[0].ln_1
        x, h = ops.layer_norm_pass(x, ln.weight, ln.bias, out_dtype=ln.out_dtype)
        for i, block in enumerate(blocks):
            nxt = blocks[i + 1].ln_1 if i + 1 < len(blocks) else tr.ln_f
            attn, mlp = block.attn, block.mlp
            qkv = ops.linear(h, attn.c_attn.weight, attn.c_attn.bias)
            ops.kv_append(qkv, kc[i], vc[i], None, 0, rows=rows)
            if prefix is None:
                y = ops.attention(qkv, attn.n_head, 0.0, False)
            else:
                y = ops.prefix_attention(qkv, self.pkc[i], self.pvc[i], prefix, attn.n_head)
            y = ops.linear(y, attn.c_proj.weight, attn.c_proj.bias)
            x, h2 = ops.add_layer_norm(x, y, block.ln_2.weight, block.ln_2.bias)
            y = mlp(h2)
            x, h = ops.add_layer_norm(x, y, nxt.weight, nxt.bias)
        return h  # ln_f(x)

    def _layers(self, tok, pos, attend, pos_inc=None):
        """The tokens ``tok`` [rows, 1] at the positions ``pos`` through the embedding, every block and
        the head -> fp32 logits [rows, 1, V].  ``attend(i, qkv)``: layer i's attention over its caches,
        the K / V append included -> c_proj's input [rows, 1, C]; ``pos_inc``: the position tensor the
        head kernel advances (None: the caller moves the positions).  Row-generic: a plain step
        feeds B rows, a speculative one B * (K + 1).

        Each linear's producer rides in its prologue at batch 1: the embedding and ln_1 in
        c_attn's (``ops.decode_embed_linear_ln``), the residual add + LayerNorm in c_attn /
        c_fc / lm_head (``ops.decode_linear_ln``), the flash-decoding combine in c_proj's
        (``decode_attention(combine=False)`` -> ``ops.decode_linear``); the K / V append
        rides in the attention kernel and bias / GELU in the GEMV epilogues: 5 launches
        per layer."""
        tr = self.model.transformer
        W = self._w  # int8 mode: the QuantWeight of a linear's weight
        branch = None  # the previous sublayer's output, not yet added to the residual x
        for i, block in enumerate(tr.h):
            attn, mlp = block.attn, block.mlp
            ln1, ln2 = block.ln_1, block.ln_2
            if i == 0:
                x, qkv = ops.decode_embed_linear_ln(tok, pos, tr.wte.weight, tr.wpe.weight, ln1.weight, ln1.bias,
                                                    W(attn.c_attn.weight), attn.c_attn.bias, dtype=self.dtype,
                                                    res_dtype=self.rdtype, out_dtype=ln1.out_dtype)
            else:
                x, qkv = ops.decode_linear_ln(x, branch, ln1.weight, ln1.bias, W(attn.c_attn.weight), attn.c_attn.bias,
                                              out_dtype=ln1.out_dtype)
            y = ops.decode_linear(attend(i, qkv), W(attn.c_proj.weight), attn.c_proj.bias)
            x, u = ops.decode_linear_ln(x, y, ln2.weight, ln2.bias, W(mlp.c_fc.weight), mlp.c_fc.bias, gelu=True,
                                        out_dtype=ln2.out_dtype)
            branch = ops.decode_linear(u, W(mlp.c_proj.weight), mlp.c_proj.bias)
        lnf = tr.ln_f
        _, logits = ops.decode_linear_ln(x, branch, lnf.weight, lnf.bias, W(self.model.lm_head.weight), None,
                                         out_f32=True, out_dtype=lnf.out_dtype, pos_inc=pos_inc)
        return logits

    def _step_impl(self):
        """The token ``tok`` at position ``pos`` through the model (``_layers``) -> fp32 logits [B, V];
        ``pos`` has advanced: by the head kernel itself, or (per_row) the unfinished rows move on and
        the finished rows stay."""
        if self.shared:
            def attend(i, qkv):
                return ops.decode_attention_shared(qkv, self.pkc[i], self.pvc[i], self.kc[i], self.vc[i], self.plen,
                                                   self.pos, self.H, append=True)
        else:
            def attend(i, qkv):
                return ops.decode_attention(qkv, self.kc[i], self.vc[i], self.pos, self.H, append=True, combine=False)
        logits = self._layers(self.tok, self.pos, attend, None if self.per_row else self.pos)
        if self.per_row:
            ops.advance_pos_(self.pos, self.done)
        return logits[:, 0]

    def _spec_step_impl(self, smp):
        """One speculative step.  The model pass: the B * (K + 1) fed tokens ``stok`` at the positions
        ``spos`` through the same embedding and linear ops as ``_step_impl`` (``_layers``; the skinny
        kernels on the GPU), with ``ops.decode_attention_spec`` in place of the single-query attention
        -> fp32 logits [B * (K + 1), V], row (b, j) for position ``pos[b] + j + 1``.  Then one draw per
        fed position with the stream the plain per-row decoder uses for it (row (b, j) hashes (b,
        pos[b] + j + 1): the sampler's ``row_key`` form over B * (K + 1) rows, into scratch), then
        ``ops.spec_accept_``: the drafts that equal their draws are kept, ``pos`` / ``tok`` / ``gen`` /
        ``done`` move on (``pos`` does not move before: every row advances by what it keeps) and the
        next step's drafts are made.  No ``advance_pos_`` and no ``pos_inc``."""
        B, S = self.B, self.K + 1

        def attend(i, qkv):
            y = ops.decode_attention_spec(qkv.view(B, S, -1), self.kc[i], self.vc[i], self.pos, self.H)
            return y.view(B * S, 1, -1)
        logits = self._layers(self.stok.view(B * S, 1), self.spos.view(B * S), attend)[:, 0]
        ops.sample_topk_(logits, smp.temperature, smp.top_k, self.salt, self.cpos.view(-1), self.ctok, self.cgen,
                         salt_dev=self.salt_dev, top_p=smp.top_p, min_p=smp.min_p, row_key=self.rkey)
        ops.spec_accept_(self.ctok.view(B, S), self.stok, self.spos, self.cpos, self.gen, self.pos, self.tok,
                         self.done, self.end, T=self.T, N=self.N, stop_token=smp.stop_token, table=self.table,
                         stats=self.spec_counts)

    def set_draft_table(self, table=None):
        """Draft from a table instead of the n-gram lookup: ``table`` (int64 [B, n] or a list of 1-D
        tensors, n <= block_size + 1) holds a guessed token for every position, the draft for position q
        being ``table[b, q]`` (positions past n: id 0).  None: back to the n-gram drafts.  For
        measuring a step at a chosen acceptance (``scripts/decode_bench.py --spec_table``) and for
        the tests: whatever the table says, the result is the plain decoder's."""
        assert self.K, "a draft table needs Decoder(..., speculate=K)"
        if table is None:
            self.table = None
            return
        if self.table is None:
            self.table = getattr(self, "_table_buf", None)
            if self.table is None:  # one buffer for the decoder's life: a captured step reads it
                self.table = self._table_buf = torch.zeros(self.B, self.T + 1, device=self.device, dtype=torch.int64)
        self.table.zero_()
        for b in range(self.B):
            row = table[b].view(-1)[:self.T + 1].to(self.device)
            self.table[b, :row.numel()] = row

    @property
    def spec_stats(self) -> dict:
        """The speculative counters since the last ``prefill``, per row: live ``steps``, drafts
        ``offered`` (per step the K drafts, or as many as the row's budget left room for) and drafts
        ``accepted``; a row's new tokens are 1 (the prefill's draw) + steps + accepted."""
        assert self.K, "spec_stats needs Decoder(..., speculate=K)"
        steps, offered, accepted = self.spec_counts.t().tolist()
        return {"steps": steps, "offered": offered, "accepted": accepted}

    def _encode(self, idx, first=0, rows=None, kc=None, vc=None):
        """``idx`` [n, S], its tokens at positions first .. first + S - 1, through the embedding and
        ``_prefill_layers`` (``first`` > 0: the suffixes of the cached prefix of that length) -> ln_f(x)."""
        tr = self.model.transformer
        wpe = tr.wpe.weight
        if first:
            wpe = ops.compute_weight(wpe, self.dtype)[first:first + idx.shape[1]]
        x = ops.embedding(idx, tr.wte.weight, wpe, 0.0, False, dtype=self.rdtype, cdtype=self.dtype)
        return self._prefill_layers(x, kc, vc, prefix=first or None, rows=rows)

    def _prefill(self, idx, first=0, lengths=None, rows=None):
        """What ``prefill``, ``prefill_suffixes`` and ``admit`` share: ``_encode``, then the rows'
        positions become ``first + lengths`` (no ``lengths``: first + S) and their finished flags 0
        (``rows``: those cache rows only, else all), and the logits of every row's last token
        [n, V] are returned."""
        n, S = idx.shape
        if lengths is not None:
            assert self.per_row, "unequal prompt lengths need Decoder(..., per_row=True)"
            lengths = torch.as_tensor(lengths, dtype=torch.int64).to(self.device).view(n)
            assert int(lengths.min()) >= 1 and int(lengths.max()) <= S
        h = self._encode(idx, first, rows)
        if self.cnt is not None:
            # the rows' histograms: rebuilt from the prompts, or (suffixes) the prefix's with the suffixes on top
            if first:
                self.cnt.copy_(self.cnt0.expand(self.B, -1))
            ops.token_counts_(self.cnt, idx, lengths, rows, accumulate=bool(first))
        if first:
            self.plen.fill_(first)
        self._lp_reset(rows)
        if rows is not None:
            self.pos.index_copy_(0, rows, lengths)
            self.done.index_fill_(0, rows, 0)
        else:
            if self.per_row:
                self.done.zero_()
            if lengths is None:
                self.pos.fill_(first + S)
            else:
                self.pos.copy_(lengths + first if first else lengths)
        if lengths is None:
            last = h[:, [-1], :]
        else:
            last = h[torch.arange(n, device=self.device), lengths - 1].unsqueeze(1)  # [n, 1, C]
        return ops.lm_head_logits(last, self.model.lm_head.weight)[:, 0]

    def _lp_reset(self, rows=None):
        """The rows' texts start over (``rows``: those rows, else all): nothing recorded yet."""
        if self.lp is None:
            return
        for t, v in ((self.lp, float("nan")), (self.top_ids, -1), (self.top_lp, float("nan")), (self.lp_last, -1)):
            if rows is None:
                t.fill_(v)
            else:
                t.index_fill_(0, rows, v)

    @torch.no_grad()
    def prefill(self, idx: torch.Tensor, lengths: torch.Tensor | None = None) -> torch.Tensor:
        """Encode the prompt [B, T0]; returns the last position's logits [B, V] (fp32).

        ``lengths`` (per_row decoders; int64 [B], 1 <= lengths[b] <= T0): ``idx`` is
        right-padded with any valid token id and row b's prompt is its first ``lengths[b]``
        tokens.  Causality keeps the padding invisible to the row's own positions, and the
        K / V rows it leaves at positions >= lengths[b] are overwritten by the step that
        feeds that position before any step reads them.  Returns the logits of position
        ``lengths[b] - 1`` of each row and sets ``pos`` to ``lengths``."""
        B, T0 = idx.shape
        assert not self.shared, "a shared_prompt decoder encodes its one prompt with prefill_shared"
        assert B == self.B and 1 <= T0 <= self.T
        if self.K:  # the drafter looks the row's own history up, prompt included
            self.gen[:, :T0] = idx
            self.spec_counts.zero_()
        return self._prefill(idx, 0, lengths)

    @torch.no_grad()
    def prefill_shared(self, idx: torch.Tensor) -> torch.Tensor:
        """Encode the one prompt ([T0] or [1, T0]) every row continues (shared_prompt decoders):
        it runs through the model as a single row, its K / V rows go to the prompt caches,
        ``plen`` becomes T0, every row's position T0 and ``done`` is cleared.  Returns the last
        position's logits as [B, V] (fp32; one row expanded: every row draws from the same
        distribution, each with its own uniform).

        The prompt's ids and those logits are kept: a later call with the same ids only puts the
        positions and flags back (``prefills`` counts the calls that ran the model), so rounds
        of samples of one prompt encode it once per decoder."""
        assert self.shared, "prefill_shared needs Decoder(..., shared_prompt=True)"
        idx = idx.reshape(1, -1).to(self.device)
        T0 = idx.shape[1]
        assert 1 <= T0 <= self.T
        if self._prompt is None or self._prompt.shape != idx.shape or not torch.equal(self._prompt, idx):
            h = self._encode(idx, kc=self.pkc, vc=self.pvc)
            self._prompt_logits = ops.lm_head_logits(h[:, [-1], :], self.model.lm_head.weight)[:, 0].float()
            self._prompt = idx.clone()
            self.prefills += 1
            if self.cnt is not None:
                ops.token_counts_(self.cnt0, idx)
        self.plen.fill_(T0)
        self.pos.fill_(T0)
        if self.per_row:
            self.done.zero_()
        self._lp_reset()
        if self.cnt is not None:
            self.cnt.copy_(self.cnt0.expand(self.B, -1))
        return self._prompt_logits.expand(self.B, -1)

    @torch.no_grad()
    def prefill_suffixes(self, idx: torch.Tensor, lengths: torch.Tensor | None = None) -> torch.Tensor:
        """Encode what every row adds to the shared prefix (after ``prefill_shared(prefix)``, P
        tokens): ``idx`` [B, S] holds row b's tokens at absolute positions P .. P + S - 1,
        right-padded with any valid id when ``lengths`` (per_row decoders; int64 [B], 1 <=
        lengths[b] <= S) says that row b's suffix is its first ``lengths[b]`` tokens.  The
        suffixes' K / V rows go to row-cache slots 0 .. S - 1 and their queries attend over the
        prompt cache plus the row's own earlier suffix keys (``ops.prefix_attention``); the
        prefix is not run again.  Padding is invisible to a row's own positions, and the rows
        it leaves in the caches are overwritten by the step that feeds that position before any
        step reads them, as after ``prefill(idx, lengths)``.  Sets ``pos`` to P + lengths (or
        P + S), clears ``done`` and returns the logits of each row's last suffix token [B, V]."""
        assert self.shared, "prefill_suffixes needs Decoder(..., shared_prompt=True)"
        assert self._prompt is not None, "prefill_suffixes follows prefill_shared(prefix)"
        B, S = idx.shape
        P = self._prompt.shape[1]
        assert B == self.B and 1 <= S <= self.R and P + S <= self.T
        return self._prefill(idx.to(self.device), P, lengths)

    def _row_index(self, rows) -> torch.Tensor:
        """``rows`` (a list or tensor of distinct cache-row indices < B) as int64 [n] on the device."""
        host = rows.tolist() if torch.is_tensor(rows) else [int(r) for r in rows]
        assert host and len(set(host)) == len(host) and all(0 <= r < self.B for r in host), \
            f"rows must be distinct indices in 0 .. {self.B - 1}, got {host}"
        return torch.tensor(host, dtype=torch.int64, device=self.device)

    @torch.no_grad()
    def admit(self, rows, idx: torch.Tensor | None = None, lengths: torch.Tensor | None = None) -> torch.Tensor:
        """Start new prompts in the cache rows ``rows`` (n distinct indices) of a running per_row
        batch; returns their last-position logits [n, V].  Every other row's caches, ``pos``,
        ``done``, ``tok``, ``gen`` and (penalising decoders) ``cnt`` stay bit for bit as they were; the
        admitted rows' ``cnt`` becomes their prompts' histograms (shared_prompt: ``cnt0``).

        Ordinary decoder: ``idx`` [n, S] holds the right-padded prompts (``lengths``: int64 [n], as in
        ``prefill``; None: every prompt has S tokens); they run through the model as a batch of
        n, the same kernels on the same shapes as ``Decoder(model, n).prefill(idx, lengths)``,
        with their K / V rows going to cache rows ``rows`` (``ops.kv_append(rows=)``: one launch
        per layer for any n).  ``pos[rows]`` becomes ``lengths`` and ``done[rows]`` 0.

        ``shared_prompt`` decoder, after ``prefill_shared``: no ``idx`` and no model pass; a row
        only goes back to the prompt's end (``pos[rows] = plen``, ``done[rows] = 0``) and the kept
        prompt logits are returned, expanded to n rows."""
        assert self.per_row, "admit needs Decoder(..., per_row=True): a position and a finished flag per row"
        rows = self._row_index(rows)
        n = rows.numel()
        if self.shared:
            assert idx is None and lengths is None, "a shared_prompt decoder admits rows of its one prompt"
            assert self._prompt is not None, "admit follows prefill_shared(prompt)"
            self.pos.index_copy_(0, rows, self.plen.expand(n))
            self.done.index_fill_(0, rows, 0)
            self._lp_reset(rows)
            if self.cnt is not None:  # nothing of the row's previous request survives
                self.cnt.index_copy_(0, rows, self.cnt0.expand(n, -1))
            return self._prompt_logits.expand(n, -1)
        assert idx is not None and idx.dim() == 2 and idx.shape[0] == n and 1 <= idx.shape[1] <= self.T
        if lengths is None:
            lengths = torch.full((n,), idx.shape[1], dtype=torch.int64, device=self.device)
        return self._prefill(idx.to(self.device), 0, lengths, rows)

    def _pen(self, smp) -> dict:
        """The sampler's penalty keywords for a draw on this decoder.  Penalising: the count table
        and the three numbers, the identity where the call passes none, so every draw is counted.
        Otherwise nothing, and a penalty that is on raises ValueError."""
        if self.cnt is None:
            if smp.penalties is not None:
                raise ValueError("sampling penalties need Decoder(..., penalize=True)")
            return {}
        rp, pp, fp = smp.penalties or (1.0, 0.0, 0.0)
        return dict(counts=self.cnt, repetition_penalty=rp, presence_penalty=pp, frequency_penalty=fp)

    def _queue_state(self):
        """``key`` and ``end`` (allocated on first use): a row that serves no request keeps key 0
        and an end position no row reaches."""
        if self.key is None:
            self.key = torch.zeros(self.B, device=self.device, dtype=torch.int64)
            self.end = torch.full((self.B,), 2 ** 62, device=self.device, dtype=torch.int64)

    @torch.no_grad()
    def sample_admitted(self, rows, logits, temperature, top_k, stop_token=None, top_p=None, min_p=None,
                        repetition_penalty=None, presence_penalty=None, frequency_penalty=None):
        """Draw the first token of the just admitted rows ``rows`` from their ``logits`` [n, V]
        (what ``admit`` returned) into ``tok`` and ``gen[b, pos[b]]``, keyed and ended by ``key`` /
        ``end`` like the queue's steps.  The sampler runs over the whole batch with every other
        row masked as finished, so those rows' ``tok``, ``gen``, ``done`` and ``cnt`` stay untouched."""
        assert self.per_row
        self._queue_state()
        smp = sampling(temperature, top_k, stop_token, top_p, min_p, repetition_penalty, presence_penalty,
                       frequency_penalty)
        pen = self._pen(smp)
        rows = self._row_index(rows)
        mask = torch.ones(self.B, device=self.device, dtype=torch.int64)
        mask.index_fill_(0, rows, 0)
        if logits.stride(0) == 0:  # one distribution for every row (shared_prompt)
            full = logits[:1].expand(self.B, -1)
        else:
            if self._admit_logits is None:
                self._admit_logits = torch.zeros(self.B, logits.shape[1], device=self.device, dtype=torch.float32)
            full = self._admit_logits
            full.index_copy_(0, rows, logits.float())
        ops.sample_topk_(full, smp.temperature, smp.top_k, self.salt, self.pos, self.tok, self.gen,
                         salt_dev=self.salt_dev, stop_token=smp.stop_token, done=mask, top_p=smp.top_p, min_p=smp.min_p,
                         row_key=self.key, end=self.end, **pen)
        self._record(full)  # the admitted rows alone: every other row's position is the one it recorded last
        self.done.index_copy_(0, rows, mask[rows])

    @torch.no_grad()
    def serve(self, prompts, budgets, temperature: float = 1.0, top_k: int | None = None,
              stop_token: int | None = None, top_p: float | None = None, min_p: float | None = None,
              repetition_penalty: float | None = None, presence_penalty: float | None = None,
              frequency_penalty: float | None = None):
        """Serve a queue of requests through the B rows of this per_row decoder, refilling a row as
        soon as its request is seen finished; returns every request's new tokens (1-D tensors, in
        request order: ``budgets[i]`` of them, or fewer, ending with ``stop_token``).

        ``prompts``: 1-D token tensors (a ``shared_prompt`` decoder: all the same one, encoded once
        by ``prefill_shared``); request i must fit, ``len(prompts[i]) + budgets[i] <= block_size``
        (a finished row is fed again at its last position, which must be a cache row), on a
        shared decoder also ``budgets[i] <=`` the row caches' slots.  The rows are filled from the
        head of the queue; then ``DONE_POLL`` steps at a time run as ``run(..., queue=True)``
        (the captured graph replayed, no host sync inside a step), ``done`` and ``pos`` are read
        back once, every finished row is harvested (``gen[b, L : pos[b] + 1]``) and the next
        prompts go into all freed rows in one ``admit`` call.  Request i samples with ``key`` i, so
        its draws depend on neither the row nor the schedule, and ends at position ``L_i + N_i -
        1`` (``end``).  ``queue_stats``: ``steps`` run, ``admissions`` (admit calls) and requests
        ``admitted``.  A decoder with ``logprobs=N`` returns ``(tokens, records)``: every request's
        ``ops.LogProbs`` is harvested with its ids, ``records[i]`` covering exactly ``tokens[i]``."""
        assert self.per_row, "serve needs Decoder(..., per_row=True)"
        if self.K:
            raise ValueError("a speculative decoder does not serve a queue")
        smp = sampling(temperature, top_k, stop_token, top_p, min_p, repetition_penalty, presence_penalty,
                       frequency_penalty)
        self._pen(smp)  # a penalty on a decoder without the table: refused before anything runs
        nreq = len(prompts)
        budgets = [int(n) for n in budgets]
        lens = [int(p.numel()) for p in prompts]
        assert len(budgets) == nreq
        for L, N in zip(lens, budgets):
            assert L >= 1 and N >= 1 and L + N <= self.T, f"a request of {L} + {N} tokens does not fit {self.T}"
            assert not self.shared or N <= self.R, f"{N} new tokens exceed the {self.R} slots of a row cache"
        self._queue_state()
        self.queue_stats = stats = {"steps": 0, "admissions": 0, "admitted": 0}
        outs: list = [None] * nreq
        if not nreq:
            return _with_records(outs, self.logprobs, [])
        B = self.B
        if self.shared:
            self.prefill_shared(prompts[0])  # every row at the prompt's end: a valid place to idle
        else:
            self.pos.zero_()
        self.done.fill_(1)  # no row serves a request yet; an idle row is a frozen one
        if self.lp is not None:
            self.lp_last.copy_(self.pos)  # ... and records nothing until it is admitted
        lps: list = [None] * nreq
        owner = [None] * B  # the request a row serves
        left = [0] * B      # an upper bound of the steps the row still needs
        nxt = 0

        def fill():
            nonlocal nxt
            free = [b for b in range(B) if owner[b] is None][:nreq - nxt]
            if not free:
                return
            reqs = list(range(nxt, nxt + len(free)))
            nxt += len(free)
            rows = torch.tensor(free, dtype=torch.int64, device=self.device)
            self.key.index_copy_(0, rows, torch.tensor(reqs, dtype=torch.int64, device=self.device))
            self.end.index_copy_(0, rows, torch.tensor([lens[i] + budgets[i] - 1 for i in reqs], dtype=torch.int64,
                                                       device=self.device))
            if self.shared:
                logits = self.admit(free)
            else:
                logits = self.admit(free, *_right_pad([prompts[i] for i in reqs], self.device))
            self.sample_admitted(free, logits, smp, None)
            for b, i in zip(free, reqs):
                owner[b], left[b] = i, budgets[i] - 1
            stats["admissions"] += 1
            stats["admitted"] += len(free)

        fill()
        while True:
            k = min(self.DONE_POLL, max(left[b] for b in range(B) if owner[b] is not None))
            if k > 0:
                self.run(k, smp, queue=True)
                stats["steps"] += k
            done, pos = torch.stack([self.done, self.pos]).tolist()  # the one host look per poll
            for b in range(B):
                i = owner[b]
                if i is None:
                    continue
                if done[b]:
                    outs[i] = self.gen[b, lens[i]:pos[b] + 1].clone()
                    if self.lp is not None:
                        lps[i] = self.records(b, lens[i], pos[b] + 1)
                    owner[b] = None
                else:
                    left[b] = lens[i] + budgets[i] - 1 - pos[b]
            fill()
            if all(o is None for o in owner):
                return _with_records(outs, self.logprobs, lps)

    @torch.no_grad()
    def step(self, tok: torch.Tensor) -> torch.Tensor:
        """Feed one token per sequence ([B] or [B, 1]) at the current position; returns
        the logits [B, V] for the next position (a view of a static buffer on the GPU)."""
        self.tok.copy_(tok.view(self.B, 1))
        if not self.use_graph:
            return self._step_impl()
        if self.graph is None:
            self.graph, self.logits = self._capture(self._step_impl)
        self.graph.replay()
        self.replays += 1
        return self.logits

    def _capture(self, fn):
        """Warm ``fn`` (a step, with or without sampling) up and record it -> (graph, what fn returned)."""
        # the warm-up: outside any graph (lazy library init, GEMM tuner decisions for M = B), at the
        # current position without advancing it or changing the fed token: the captured
        # step rewrites the same cache rows when it runs, and whatever else a step writes
        # (``_written``) is put back
        saved = [(t, t.clone()) for t in self._written()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                fn()
                for t, was in saved:
                    t.copy_(was)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):  # recorded, not executed: pos is unchanged
            out = fn()
        return graph, out

    def _written(self) -> list:
        """The tensors a step, with or without sampling, writes beside the caches and ``gen``, for this
        decoder's mode: the fed token and the position; the finished flags (a warm-up draw may hit the
        stop token); a speculative step also accepts and drafts (its fed tokens, their positions and
        the counters); a penalising decoder counts the draw (the table) and one with ``logprobs``
        records it (the records and the marker)."""
        return ([self.tok, self.pos] + ([self.done] if self.per_row else [])
                + ([self.stok, self.spos, self.cpos, self.spec_counts] if self.K else [])
                + ([self.cnt] if self.cnt is not None else [])
                + ([self.lp, self.top_ids, self.top_lp, self.lp_last] if self.lp is not None else []))

    def sample_into(self, logits, temperature, top_k, stop_token=None, top_p=None, min_p=None, queue=False,
                    repetition_penalty=None, presence_penalty=None, frequency_penalty=None):
        """Draw the next token of every row from ``logits`` [B, V] into ``tok`` and
        ``gen[:, pos]`` (device kernel on the GPU: ``ops.sample_topk_``).  per_row: row b
        writes ``gen[b, pos[b]]``; a finished row draws nothing, and a row that draws
        ``stop_token`` is finished from then on.  ``top_p`` / ``min_p``: nucleus and min-p
        filters on top of the top-k (off: the top-k sampler's own launch).  ``queue``: the
        serving queue's form, every row keyed by ``key`` and finished at ``end``.  The three
        penalties (penalising decoders; None: off): the draw is made from
        ``ops.penalize_logits(logits, cnt, ...)`` and counted in ``cnt``, inside the same launch."""
        smp = sampling(temperature, top_k, stop_token, top_p, min_p, repetition_penalty, presence_penalty,
                       frequency_penalty)
        if queue:
            assert self.per_row and self.key is not None, "the queue form needs a per_row decoder with key / end"
        assert smp.stop_token is None or self.per_row, "a stop token needs Decoder(..., per_row=True)"
        # ``done`` is None without per_row, ``key`` / ``end`` are passed by the queue only: the sampler
        # picks its entry point from what is there
        ops.sample_topk_(logits, smp.temperature, smp.top_k, self.salt, self.pos, self.tok, self.gen,
                         salt_dev=self.salt_dev, stop_token=smp.stop_token, done=self.done, top_p=smp.top_p,
                         min_p=smp.min_p, row_key=self.key if queue else None, end=self.end if queue else None,
                         **self._pen(smp))
        self._record(logits)

    def _record(self, logits):
        """logprobs: the log-probability of the token every row has just drawn from the raw ``logits``
        [B, V], and the alternatives, at ``pos`` (``ops.token_logprobs_step_``: one launch)."""
        if self.lp is not None:
            ops.token_logprobs_step_(logits, self.tok, self.pos, self.lp_last, self.lp, self.top_ids, self.top_lp,
                                     V=self.model.config.vocab_size)

    def reseed(self):
        """A fresh sampling stream for the next generate call (torch.manual_seed governs)."""
        self.salt_dev.fill_(int(torch.randint(0, 2 ** 62, (1,)).item()))

    def _step_sample_impl(self, smp, queue=False):
        self.sample_into(self._step_impl(), smp, None, queue=queue)  # pos is now p + 1

    def _replay(self, step, smp, queue=False):
        """What ``run`` calls per token: ``step`` itself (eager), or the replay of its captured graph,
        captured on first use under the step's ``graph_key``."""
        if not self.use_graph:
            return step
        key = graph_key(smp, self.per_row, queue, (self.K, self.N) if self.K else None,
                        bool(self.K) and self.table is not None, self.cnt is not None, self.logprobs)
        if key not in self.sgraphs:
            self.sgraphs[key], _ = self._capture(step)
        return self.sgraphs[key].replay

    DONE_POLL = 16  # run(): replays between two host looks at the finished flags

    @torch.no_grad()
    def run(self, n: int, temperature: float = 1.0, top_k: int | None = None, stop_token: int | None = None,
            top_p: float | None = None, min_p: float | None = None, queue: bool = False,
            repetition_penalty: float | None = None, presence_penalty: float | None = None,
            frequency_penalty: float | None = None):
        """Decode n tokens starting from ``self.tok`` at ``self.pos``: each step feeds the
        token, samples the next one and feeds it back on the device (one graph replay per
        token on the GPU, no host round trip).  Results land in ``self.gen``.  With a
        ``stop_token`` (per_row decoders) the finished flags are read back every
        ``DONE_POLL`` steps and the loop ends early once every row has finished.  ``queue``
        (``serve``): the sampler reads ``key`` and ``end``, a graph of its own (the key gains
        ``"queue"``); without it the graphs and their keys are the ones there always were.  The
        three penalties: as in ``sample_into``; on a penalising decoder the key gains ``("pen", rp,
        pp, fp)``, the identity (1, 0, 0) when none is passed.  A decoder with ``logprobs=N`` records
        every draw (``lp`` / ``top_ids`` / ``top_lp``) and its key gains ``("lp", N)``."""
        smp = sampling(temperature, top_k, stop_token, top_p, min_p, repetition_penalty, presence_penalty,
                       frequency_penalty)
        assert smp.stop_token is None or self.per_row, "a stop token needs Decoder(..., per_row=True)"
        self._pen(smp)  # a penalty on a decoder without the table: refused here, whatever n and the mode
        if self.K:
            if queue:
                raise ValueError("a speculative decoder does not serve a queue")
            return self._run_spec(n, smp)
        step = self._replay(lambda: self._step_sample_impl(smp, queue), smp, queue)
        stop_token = smp.stop_token
        ran = 0
        while ran < n:
            if stop_token is not None and ran and ran % self.DONE_POLL == 0 and bool(self.done.all()):
                break
            step()
            ran += 1
        if self.use_graph:
            self.replays += ran

    def _run_spec(self, n, smp):
        """``run`` on a speculative decoder: every unfinished row gets n more tokens (``end`` = its
        position + n), the first drafts are made, and the step (``_spec_step_impl``, captured once per
        sampling key with ``("spec", K, N)`` added) is replayed until every row is done, looked for
        every ``DONE_POLL`` replays: at most n of them, since a live step emits at least one token."""
        if n <= 0:
            return
        self.end.copy_(torch.clamp(self.pos + n, max=self.T))
        ops.ngram_draft(self.gen, self.pos, self.tok, self.K, self.N, self.T, self.table,
                        out=(self.stok, self.spos, self.cpos))
        step = self._replay(lambda: self._spec_step_impl(smp), smp)
        # between two host looks: DONE_POLL replays, or fewer when the rows cannot need that many (a row
        # that is ``left`` tokens short needs at least ceil(left / (K + 1)) more steps), so the tail of a
        # well-drafted run is not padded with idle replays
        ran, left = 0, n
        while left > 0 and ran < n:
            k = min(self.DONE_POLL, -(-left // (self.K + 1)), n - ran)
            for _ in range(k):
                step()
            ran += k
            done, pos, end = torch.stack([self.done, self.pos, self.end]).tolist()  # the one host look per poll
            left = max([e - p for d, p, e in zip(done, pos, end) if not d], default=0)
        if self.use_graph:
            self.replays += ran

    def records(self, rows, first: int, stop: int) -> "ops.LogProbs":
        """A copy of what was recorded for positions first .. stop - 1 of ``rows`` (an index or a slice)."""
        assert self.lp is not None, "records needs Decoder(..., logprobs=N)"
        return ops.LogProbs(self.lp[rows, first:stop].clone(), self.top_ids[rows, first:stop].clone(),
                            self.top_lp[rows, first:stop].clone())

    @property
    def position(self) -> int:
        return int(self.pos.item())

    @property
    def positions(self) -> list[int]:
        """Every row's position (per_row decoders; the shared position repeated otherwise)."""
        p = self.pos.tolist()
        return p if self.per_row else p * self.B


def sample_next(logits: torch.Tensor, temperature: float = 1.0, top_k: int | None = None,
                generator: torch.Generator | None = None, top_p: float | None = None,
                min_p: float | None = None, counts: torch.Tensor | None = None,
                repetition_penalty: float | None = None, presence_penalty: float | None = None,
                frequency_penalty: float | None = None) -> torch.Tensor:
    """nanoGPT's sampling: logits / temperature, optional top-k (None or 0: off), nucleus
    ``top_p`` and ``min_p`` (``ops.filter_logits``), softmax, multinomial -> [B, 1].  With
    ``counts`` ([B, >= V]: how often every id occurs in the row's whole text) the raw logits are
    penalised first (``ops.penalize_logits``); ``counts`` itself is the caller's to update."""
    _, _, _, top_p, min_p, pen = sampling(temperature, top_k, None, top_p, min_p, repetition_penalty, presence_penalty,
                                          frequency_penalty)
    if pen is not None:
        if counts is None:
            raise ValueError("sampling penalties need counts")
        logits = ops.penalize_logits(logits, counts, *pen)
    logits = logits.float() / temperature
    if top_k:
        v, _ = torch.topk(logits, min(top_k, logits.size(-1)))
        logits = logits.masked_fill(logits < v[:, -1:], -float("Inf"))  # basic slicing: capturable
    if top_p is not None or min_p is not None:
        logits = ops.filter_logits(logits, None, top_p, min_p)
    probs = torch.softmax(logits, dim=-1)
    return torch.multinomial(probs, num_samples=1, generator=generator)


def _mode(B, per_row=False, quantize=None, kv_quantize=None, slots=None, spec=(0, 3), penalize=False,
          logprobs=None) -> dict:
    """The decoder a call needs, as ``Decoder``'s arguments (and ``Decoder.fits``'s): B rows, per_row
    or not, the two quantizations, ``slots``, the row-cache slots of a shared_prompt decoder
    (None: an unshared one), ``spec``, the (K, N) of ``_check`` (K > 0: a speculative one, which
    is per_row), ``penalize``: one with a count table, for a call with a penalty on, and ``logprobs``:
    one with the log-probability buffers of that many alternatives (None: without).  ``_check`` has
    refused what does not compose."""
    K, N = spec
    return dict(batch_size=B, per_row=per_row or bool(K), quantize=quantize, kv_quantize=kv_quantize,
                shared_prompt=slots is not None, max_new=slots, speculate=K or None, spec_ngram=N,
                penalize=bool(penalize), logprobs=logprobs)


def _build(model, mode, use_graph=None):
    return Decoder(model, max_len=model.config.block_size, use_graph=use_graph, **mode)


@contextlib.contextmanager
def _borrow(model, mode, decoder, use_graph):
    """The decoder a call of ``mode`` runs on, reseeded: the caller's ``decoder`` if it fits (its
    weight shadows, captured graphs and cached prompt survive; the caller releases it), otherwise
    a temporary one, released on exit."""
    own = decoder is None or not decoder.fits(**mode)
    dec = _build(model, mode, use_graph) if own else decoder
    try:
        dec.reseed()  # every call draws its own samples, also on a reused decoder / graph
        yield dec
    finally:
        if own:
            dec.release()


def _nothing_to_share(sharing, L, N, T):
    return ValueError(f"{sharing} needs the KV-cache path: prompt ({L}) + new tokens ({N}) exceed block_size {T}, "
                      "and the recompute loop has nothing to share")


def _cached_mode(model, idx, max_new_tokens, quantize, kv_quantize, shared_prompt, speculate=None, spec_ngram=3,
                 penalize=False, logprobs=None):
    """``generate_cached``'s plan -> (mode, cached): the mode of the decoder the call runs on, validated
    (``_check``), or ``cached`` False: no new tokens, or the recompute loop, and ``mode`` is the
    ordinary decoder's all the same.  ``penalize``: the call has a penalty on; ``logprobs``: it wants the
    log-probabilities."""
    K, N, logprobs = _check(quantize, kv_quantize, shared_prompt, speculate=speculate, spec_ngram=spec_ngram,
                            penalize=penalize, logprobs=logprobs)
    B, T0 = idx.shape
    T = model.config.block_size
    plain = _mode(B, False, quantize, kv_quantize, spec=(K, N), penalize=penalize, logprobs=logprobs)
    if max_new_tokens <= 0:
        return plain, False
    if shared_prompt:
        if not bool((idx == idx[:1]).all()):
            raise ValueError("shared_prompt needs every row of idx to be the same prompt")
        if B > 1:  # a single row goes the ordinary way
            if T0 + max_new_tokens > T:
                raise _nothing_to_share("shared_prompt", T0, max_new_tokens, T)
            return _mode(B, False, quantize, slots=max_new_tokens, penalize=penalize, logprobs=logprobs), True
    if T0 + max_new_tokens - 1 > T:
        if quantize:
            raise ValueError("quantize needs the KV-cache path: prompt + new tokens exceed block_size, and the "
                             "recompute loop runs the unquantized model")
        if kv_quantize:
            raise ValueError("kv_quantize needs the KV-cache path: prompt + new tokens exceed block_size, and the "
                             "recompute loop has no cache to quantize")
        if K:
            raise ValueError("speculate needs the KV-cache path: prompt + new tokens exceed block_size, and the "
                             "recompute loop decodes one token per pass")
        return plain, False
    return plain, True


def cached_decoder(model, idx, max_new_tokens, use_graph=None, quantize=None, kv_quantize=None, shared_prompt=False,
                   speculate=None, spec_ngram=3, repetition_penalty=None, presence_penalty=None,
                   frequency_penalty=None, logprobs=None):
    """The Decoder this ``generate_cached`` call would build, for a caller that keeps it across
    calls (``decoder=``) and releases it.  A call that runs on none (no new tokens, or the
    recompute loop) gets the ordinary one all the same, as ``sample.py`` always has: building it
    draws from torch's generator, and a seeded run keeps its tokens.  With a penalty on it is a
    penalising one, with ``logprobs`` one that records them."""
    pen = sampling_penalties(repetition_penalty, presence_penalty, frequency_penalty) is not None
    return _build(model, _cached_mode(model, idx, max_new_tokens, quantize, kv_quantize, shared_prompt, speculate,
                                      spec_ngram, pen, logprobs)[0], use_graph)


@torch.no_grad()
def generate_cached(model, idx: torch.Tensor, max_new_tokens: int, temperature: float = 1.0,
                    top_k: int | None = None, use_graph: bool | None = None,
                    decoder: "Decoder | None" = None, top_p: float | None = None,
                    min_p: float | None = None, quantize: str | None = None,
                    kv_quantize: str | None = None, shared_prompt: bool = False,
                    speculate: int | None = None, spec_ngram: int = 3, spec_table=None,
                    repetition_penalty: float | None = None, presence_penalty: float | None = None,
                    frequency_penalty: float | None = None, logprobs: int | None = None):
    """``model.generate`` with KV caches: same sampling, one token's forward per new token.

    ``logprobs=N`` (0 .. 8; None: off): the call returns ``(tokens, ops.LogProbs)``, the second covering
    exactly the new tokens: ``token`` [B, n] is the log-probability of every drawn token under the
    model's raw logits (before penalties, temperature and filters; ``ops.token_logprobs``), ``top_ids`` /
    ``top`` [B, n, N] the N most likely ids and theirs.  It runs on a decoder that records them
    (``Decoder(..., logprobs=N)``: one more launch per token, inside the captured step; the tokens are
    those of the call without it), past block_size the recompute loop fills it through the same op.
    ValueError with ``speculate``.  Without the keyword the return value is the tokens alone.

    ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty`` (``ops.penalize_logits``; 1, 0
    and 0 or None: off): with one of them on the call runs on a penalising decoder
    (``Decoder(..., penalize=True)``: built here, or ``decoder`` if it is one), whose sampler applies
    them to the raw logits inside its one launch, from counts of the row's prompt and drawn tokens.
    Past block_size the recompute loop applies the same rule.  ValueError with ``speculate``.

    ``speculate=K`` (1 .. 7): speculative decoding (``Decoder(..., speculate=K, spec_ngram=N)``). A
    step feeds every row's token and K continuations guessed by n-gram lookup in the row's own
    history, draws the token of every fed position with the stream the plain decoder uses for it
    and keeps the drafts that equal their draws: up to K + 1 tokens per model pass, and the same
    tokens as without it.  ``spec_table`` ([B, n] ids by position) drafts from a table instead
    (``Decoder.set_draft_table``).  ValueError with ``kv_quantize``, ``shared_prompt``, prompt + new
    tokens past block_size and, on the GPU, B * (K + 1) > 16 or a model without the fused decode
    kernels.

    ``shared_prompt=True``: the rows of ``idx`` are one prompt (unequal rows raise ValueError)
    whose K / V are cached once for the batch (``Decoder(..., shared_prompt=True)``); a single
    row goes the ordinary way.  No recompute fallback: prompt + new tokens past block_size
    raise ValueError, and so does ``kv_quantize``.

    ``quantize="int8"``: decode with int8 weights (``Decoder(..., quantize="int8")``); the
    recompute fallback cannot, so a prompt + new tokens past block_size raises ValueError.
    ``kv_quantize="int8"``: int8 KV caches (``Decoder(..., kv_quantize="int8")``); the
    recompute loop has no cache, so the same case raises ValueError as well.

    ``decoder``: a Decoder to reuse across calls (same batch size and form; ``cached_decoder``
    builds the one a call needs): its weight shadows and captured graphs survive, so
    ``sample.py``'s num_samples loop captures once.  The caller releases it; without one, or
    with one that does not fit, a temporary decoder is built and released here."""
    T0 = idx.shape[1]
    smp = sampling(temperature, top_k, None, top_p, min_p, repetition_penalty, presence_penalty, frequency_penalty)
    mode, cached = _cached_mode(model, idx, max_new_tokens, quantize, kv_quantize, shared_prompt, speculate, spec_ngram,
                                smp.penalties is not None, logprobs)
    logprobs = mode["logprobs"]
    if max_new_tokens <= 0:
        return _with_records(idx, logprobs, lambda: _no_records(idx.shape[0], logprobs, idx.device))
    if not cached:
        # the caches hold block_size positions; nanoGPT crops the context beyond that
        rp, pp, fp = smp.penalties or (None, None, None)
        return model.generate(idx, max_new_tokens, temperature=smp.temperature, top_k=smp.top_k, top_p=smp.top_p,
                              min_p=smp.min_p, repetition_penalty=rp, presence_penalty=pp, frequency_penalty=fp,
                              logprobs=logprobs)
    with _borrow(model, mode, decoder, use_graph) as dec:
        if dec.K:
            dec.set_draft_table(spec_table)
        logits = dec.prefill_shared(idx[0]) if dec.shared else dec.prefill(idx)
        dec.sample_into(logits, smp, None)  # pos = T0: gen[:, T0]
        dec.run(max_new_tokens - 1, smp)
        out = torch.cat([idx, dec.gen[:, T0:T0 + max_new_tokens]], dim=1)
        return _with_records(out, logprobs, lambda: dec.records(slice(None), T0, T0 + max_new_tokens))


def _with_records(out, logprobs, records):
    """What a call returns: ``out`` if ``logprobs`` is off, otherwise ``(out, records)``; ``records`` may be a
    function that makes them, called only then."""
    return out if logprobs is None else (out, records() if callable(records) else records)


def _no_records(B, N, device) -> "ops.LogProbs":
    """The records of no new tokens."""
    return ops.LogProbs(torch.zeros(B, 0, device=device), torch.zeros(B, 0, N, dtype=torch.int32, device=device),
                        torch.zeros(B, 0, N, device=device))


def _right_pad(prompts, device):
    """1-D ``prompts`` as one right-padded (any valid id) int64 [n, longest] and their lengths [n]."""
    lens = [p.numel() for p in prompts]
    idx = torch.zeros(len(prompts), max(lens), dtype=torch.int64, device=device)
    for b, p in enumerate(prompts):
        idx[b, :lens[b]] = p
    return idx, torch.tensor(lens, dtype=torch.int64, device=device)


def _result(prompt, new, stop_token=None) -> torch.Tensor:
    """The prompt followed by its new tokens, those up to and including the first ``stop_token``."""
    if stop_token is not None:
        hit = (new == stop_token).nonzero()
        if hit.numel():
            new = new[:int(hit[0]) + 1]
    return torch.cat([prompt, new])


def common_prefix_len(prompts) -> int:
    """The prefix length P a shared_prefix batch caches once: the longest common token prefix of
    the 1-D ``prompts``, but at most the shortest prompt - 1, so every row keeps a suffix token."""
    n = min(p.numel() for p in prompts) - 1
    if n <= 0 or len(prompts) < 2:
        return max(n, 0)
    first = prompts[0][:n]
    same = torch.stack([p[:n].to(first.device) == first for p in prompts[1:]]).all(dim=0)
    return int(same.long().cumprod(0).sum())


def _batch_plan(model, prompts, max_new_tokens, quantize, kv_quantize, shared_prompt, shared_prefix, batch_size,
                speculate=None, spec_ngram=3, penalize=False, logprobs=None):
    """What ``generate_batch`` does with a call -> (prompts, budgets, queue, fit, P, mode): the
    flattened prompts on the model's device, every prompt's budget of new tokens, whether they are
    served as a queue, the indices of the prompts that share the decoder (the others go alone), the
    length of the prefix they share through ``prefill_suffixes`` (0: none) and the decoder's mode,
    validated (``_check``; no prompt fits: the ordinary one of a row per prompt all the same).  ``budgets``
    None: there is nothing to generate."""
    queue = batch_size is not None or not isinstance(max_new_tokens, int)
    if queue:
        if batch_size is not None and (not isinstance(batch_size, int) or batch_size < 1):
            raise ValueError(f"batch_size must be a positive int, got {batch_size!r}")
        if shared_prefix:
            raise ValueError("shared_prefix batches are not served as a queue: drop batch_size / per-prompt budgets")
        if not isinstance(max_new_tokens, int):
            budgets = [int(n) for n in max_new_tokens]
            if len(budgets) != len(prompts):
                raise ValueError(f"{len(budgets)} budgets for {len(prompts)} prompts")
            if any(n < 1 for n in budgets):
                raise ValueError(f"every budget must be at least 1, got {budgets}")
    *spec, logprobs = _check(quantize, kv_quantize, shared_prompt, shared_prefix, queue, speculate, spec_ngram,
                             penalize, logprobs)
    plain = _mode(len(prompts), True, quantize, kv_quantize, spec=spec, penalize=penalize, logprobs=logprobs)
    assert all(p.numel() >= 1 for p in prompts), "every prompt needs at least one token"
    device = model.lm_head.weight.device
    prompts = [p.view(-1).to(device) for p in prompts]
    if shared_prompt and any(p.shape != prompts[0].shape or not torch.equal(p, prompts[0]) for p in prompts[1:]):
        raise ValueError("shared_prompt needs every prompt to be the same")
    if isinstance(max_new_tokens, int):
        if max_new_tokens <= 0:
            return prompts, None, queue, [], 0, plain
        budgets = [max_new_tokens] * len(prompts)
    T = model.config.block_size
    P = common_prefix_len(prompts) if shared_prefix and len(prompts) > 1 else 0  # one prompt, no prefix: ordinary
    sharing = "shared_prefix" if P else "shared_prompt" if shared_prompt and (queue or len(prompts) > 1) else None
    # an ordinary batch's last new token is drawn and never fed, so it needs no cache row; a queue's finished
    # row idles at its last position, which must be a cache row: a request that does not fit so goes alone
    spare = 0 if queue or sharing else 1
    fit = [i for i, p in enumerate(prompts) if p.numel() + budgets[i] - spare <= T]
    if sharing:
        for i, p in enumerate(prompts):
            if i not in fit:
                raise _nothing_to_share(sharing, p.numel(), budgets[i], T)
    if not fit:
        return prompts, budgets, queue, fit, P, plain
    B = len(fit) if batch_size is None else min(batch_size, len(fit))
    slots = None
    if sharing and B >= 2:  # a single row goes the ordinary way
        # a row's cache holds what follows the shared tokens: its suffix, if any, and its new tokens
        slots = max(budgets[i] + (prompts[i].numel() - P if P else 0) for i in fit)
    return prompts, budgets, queue, fit, P, _mode(B, True, quantize, kv_quantize, slots, spec, penalize, logprobs)


def batch_decoder(model, prompts, max_new_tokens, use_graph=None, quantize=None, kv_quantize=None,
                  shared_prompt=False, shared_prefix=False, batch_size=None, speculate=None, spec_ngram=3,
                  repetition_penalty=None, presence_penalty=None, frequency_penalty=None, logprobs=None):
    """The Decoder this ``generate_batch`` call would build, for a caller that keeps it across
    calls (``decoder=``; a shared one then keeps the prompt or prefix too) and releases it.  A call
    that shares none (no new tokens, or no prompt that fits the cache) gets the ordinary one of a
    row per prompt, for the reason ``cached_decoder`` gives.  With a penalty on it is a penalising one."""
    pen = sampling_penalties(repetition_penalty, presence_penalty, frequency_penalty) is not None
    mode = _batch_plan(model, prompts, max_new_tokens, quantize, kv_quantize, shared_prompt, shared_prefix, batch_size,
                       speculate, spec_ngram, pen, logprobs)[-1]
    return _build(model, mode, use_graph)


@torch.no_grad()
def generate_batch(model, prompts, max_new_tokens, temperature: float = 1.0, top_k: int | None = None,
                   stop_token: int | None = None, use_graph: bool | None = None,
                   decoder: "Decoder | None" = None, top_p: float | None = None,
                   min_p: float | None = None, quantize: str | None = None,
                   kv_quantize: str | None = None, shared_prompt: bool = False,
                   shared_prefix: bool = False, batch_size: int | None = None, speculate: int | None = None,
                   spec_ngram: int = 3, spec_table=None, repetition_penalty: float | None = None,
                   presence_penalty: float | None = None, frequency_penalty: float | None = None,
                   logprobs: int | None = None):
    """Generate for a list of prompts of unequal lengths as one batch.

    ``logprobs=N`` (0 .. 8; None: off): as in ``generate_cached``; the call returns ``(results, records)``,
    ``records[i]`` the ``ops.LogProbs`` of prompt i's new tokens (``token`` [n_i], ``top_ids`` / ``top`` [n_i, N]),
    trimmed through the stop token as the ids are, so the stop token's own log-probability is its
    last entry.  A queue harvests a request's records with its ids.  ValueError with ``speculate``.

    ``repetition_penalty`` / ``presence_penalty`` / ``frequency_penalty``: as in ``generate_cached``; every
    row is penalised by the counts of its own prompt (prefix and suffix) and drawn tokens, a queue's
    row by those of the request it serves.  ValueError with ``speculate``.

    ``speculate=K`` / ``spec_ngram=N`` / ``spec_table``: speculative decoding, as in
    ``generate_cached`` (``spec_table``: one 1-D tensor of ids by position per prompt); every row
    advances by what it accepts, and the results are those of the call without it.  ValueError with
    ``kv_quantize``, ``shared_prompt``, ``shared_prefix`` and a queue (``batch_size`` / per-prompt
    budgets); a row that does not fit the cache goes alone, speculating too.

    ``prompts``: 1-D token tensors, each of length >= 1.  Every result is its prompt followed
    by the new tokens: up to and including the first ``stop_token`` if the row drew it,
    otherwise exactly ``max_new_tokens`` of them.  The rows share one per_row ``Decoder``
    (right-padded prefill, then one step per token for the whole batch, every row at its
    own position; a row that has drawn the stop token is frozen).  A row whose prompt +
    new tokens exceed block_size cannot live in the cache: it goes through
    ``generate_cached`` on its own (the recompute loop) and is cut at the stop token.

    ``decoder``: a per_row Decoder of the right batch size to reuse across calls (weight
    shadows and captured graphs survive; ``batch_decoder`` builds the one a call needs); the
    caller releases it.  ``quantize="int8"``: int8 weights; a row that needs the recompute
    loop then raises ValueError.
    ``kv_quantize="int8"``: int8 KV caches, with the same refusal.

    ``shared_prompt=True``: every prompt must be the same one (ValueError otherwise); it is
    encoded once, as a single row, into a prompt cache the whole batch attends over, and each
    row caches only its own new tokens (``Decoder(..., shared_prompt=True, max_new=
    max_new_tokens)``; ``decoder`` is reused only if it is such a one, and then keeps the
    prompt between calls).  A single prompt goes the ordinary way.  Prompt + new tokens past
    block_size and ``kv_quantize`` raise ValueError.

    ``shared_prefix=True``: the prompts share a prefix (a system prompt followed by different
    questions).  P = the longest common token prefix, at most the shortest prompt - 1 so that
    every row keeps a suffix token (``common_prefix_len``); the prefix is encoded once, as a
    single row, into the prompt caches, the suffixes are prefilled against it
    (``Decoder.prefill_suffixes``) and every row caches its suffix and its new tokens only
    (``Decoder(..., shared_prompt=True, per_row=True, max_new=longest suffix +
    max_new_tokens)``; ``decoder`` is reused only if it is such a one, and then keeps the
    prefix between calls).  One prompt, or no common prefix: the ordinary path.  ``kv_quantize``,
    ``shared_prompt=True`` at the same time and a row whose prompt + new tokens exceed
    block_size raise ValueError.

    ``batch_size`` (and / or ``max_new_tokens`` as one budget per prompt): the prompts are a
    queue served in order through min(batch_size, number of prompts) rows; a row whose request
    has finished (its own budget, or the stop token) is given the next prompt (``Decoder.serve``:
    finished rows are looked for every ``DONE_POLL`` steps and all freed rows are admitted in one
    prefill pass), so neither the decoder nor the time grows with the longest request of a
    chunk.  Results come back in prompt order, in the form above.  Sampling is keyed by the
    request, not the row.  An admission's prefill shape depends on the schedule, so on the GPU
    its logits may differ from a chunked run's in the last bf16 bits; with ``shared_prompt=True``
    (the same prompt everywhere, at least 2 rows; admission costs nothing, one prefill) nothing
    does, and the results do not depend on the schedule.  A request must fit the cache with one
    row to spare, prompt + budget <= block_size: one that does not goes alone through
    ``generate_cached`` (``quantize`` / ``kv_quantize`` / ``shared_prompt``: ValueError).
    ``shared_prefix=True``, ``batch_size < 1`` and a budget list of the wrong length or with an
    entry < 1 raise ValueError.  With ``batch_size=None`` and an int budget nothing changes."""
    smp = sampling(temperature, top_k, stop_token, top_p, min_p, repetition_penalty, presence_penalty,
                   frequency_penalty)
    given = prompts
    prompts, budgets, queue, fit, P, mode = _batch_plan(model, prompts, max_new_tokens, quantize, kv_quantize,
                                                        shared_prompt, shared_prefix, batch_size, speculate,
                                                        spec_ngram, smp.penalties is not None, logprobs)
    logprobs = mode["logprobs"]
    if budgets is None:
        outs = [p.view(-1) for p in given]
        return _with_records(outs, logprobs, lambda: [_row(_no_records(1, logprobs, p.device), 0, 0) for p in outs])
    outs: list = [None] * len(prompts)
    lps: list = [None] * len(prompts)
    for i, p in enumerate(prompts):
        if i not in fit:  # alone through ``generate_cached``: the recompute loop, or a decoder of its own
            y = generate_cached(model, p[None], budgets[i], smp._replace(stop_token=None), use_graph=use_graph,
                                quantize=quantize, kv_quantize=kv_quantize, speculate=speculate, spec_ngram=spec_ngram,
                                spec_table=None if spec_table is None else [spec_table[i]], logprobs=logprobs)
            if logprobs is not None:
                y, rec = y
            outs[i] = _result(p, y[0][p.numel():], smp.stop_token)
            if logprobs is not None:
                lps[i] = _row(rec, 0, outs[i].numel() - p.numel())
    if not fit:
        return _with_records(outs, logprobs, lps)
    with _borrow(model, mode, decoder, use_graph) as dec:
        if queue:
            news = dec.serve([prompts[i] for i in fit], [budgets[i] for i in fit], smp)
            if logprobs is not None:
                news, recs = news
        else:
            if P:
                dec.prefill_shared(prompts[0][:P])
                logits = dec.prefill_suffixes(*_right_pad([p[P:] for p in prompts], dec.device))
            elif dec.shared:
                logits = dec.prefill_shared(prompts[0])
            else:
                if dec.K:
                    dec.set_draft_table(None if spec_table is None else [spec_table[i] for i in fit])
                logits = dec.prefill(*_right_pad([prompts[i] for i in fit], dec.device))
            dec.sample_into(logits, smp, None)  # gen[b, its prompt's length]
            dec.run(max_new_tokens - 1, smp)
        for b, i in enumerate(fit):
            L = prompts[i].numel()
            outs[i] = (_result(prompts[i], news[b]) if queue else
                       _result(prompts[i], dec.gen[b, L:L + max_new_tokens], smp.stop_token))
            if logprobs is not None:  # exactly the new tokens, through the stop token
                lps[i] = recs[b] if queue else dec.records(b, L, outs[i].numel())
    return _with_records(outs, logprobs, lps)


def _row(rec, b, n) -> "ops.LogProbs":
    """Row b of batched records, its first n entries."""
    return ops.LogProbs(rec.token[b, :n], rec.top_ids[b, :n], rec.top[b, :n])


