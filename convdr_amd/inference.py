"""Query-encode loop of the retrieval driver on MI355X.

Mirrors /root/reference/drivers/run_convdr_inference.py:116-154 (``evaluate``), same signature and return value:
the eval set is walked in order in batches of ``per_gpu_eval_batch_size * max(1, n_gpu)``, every batch is encoded by
``model(concat_ids, concat_id_mask)`` (the HIP encoder behind ``model.models``), and the function returns
``(embedding float32 [N, 768] numpy, embedding2id list of query ids, raw_sequences list of history utterances)``.

What changed for the GPU (results identical): the reference copies every batch's embeddings to the host synchronously
(``embs.detach().cpu().numpy()`` per batch, :145); here the batches stay on the device and come back in ONE copy after the
loop, so the host keeps enqueueing while the GPU encodes (query batches are 4 x <= 510 tokens: launch-bound).

Extension, opt-in (``token_budget=`` or ``args.eval_token_budget``): the forward of one 4-query batch is ~70 launches over a
few hundred packed rows.  With a budget the DataLoader is walked exactly as before, but the kept tokens of its batches are
flattened on the host into one int32 stream and the sequences accumulate ACROSS batches into groups of at most `token_budget`
packed rows (the cut of ``encode.plan_batches`` over the dataset order); each group is one upload and one forward through
the ragged encoder entry (``model.query_emb_ragged`` -> convdr_encoder_forward_ragged).  A group is enqueued as soon as the
next sequence would overflow it, so the set is never materialised.  ``last_evaluate_stats`` records what the last call did.
"""
import random

import numpy as np
import torch
from torch.utils.data import DataLoader, SequentialSampler


def set_seed(args):
    """utils/util.py:233-238."""
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    if getattr(args, "n_gpu", 0) > 0 and torch.cuda.is_available():
        torch.cuda.manual_seed_all(args.seed)


last_evaluate_stats = {}      # of the last evaluate() call: forwards, groups [(first, end)], padded_batches, token_budget


def _flatten_prefix_batch(ids, mask):
    """A padded batch (numpy [B, L] ids and 0/1 mask) -> (tokens int32 [mask.sum()], lens int32 [B]): the kept tokens of
    its rows back to back, in row order.  None when some row's mask is not a prefix (a 0 followed by a 1): such a batch is
    not representable as a stream (the masked ids in front of kept ones enter RoBERTa's position count)."""
    ids, keep = np.asarray(ids), np.asarray(mask) != 0
    lens = keep.sum(1).astype(np.int32)
    prefix = np.arange(keep.shape[1])[None, :] < lens[:, None]
    if not np.array_equal(keep, prefix):
        return None
    return np.ascontiguousarray(ids[prefix], dtype=np.int32), lens


class _GroupCutter:
    """Streaming form of ``encode.plan_batches(lens, N, token_budget, align)``: sequences are announced one by one, in
    order; a group closes when the next sequence would take it past the budget (each sequence counted as its length rounded
    up to `align`, a single longer one forming a group of its own)."""

    def __init__(self, token_budget, align=8):
        self.budget, self.align = int(token_budget), int(align)
        self.first = self.end = self.used = 0

    def add(self, n):
        """Announce the next sequence (n tokens) -> the group (first, end) that had to be closed in front of it, or None."""
        a = (int(n) + self.align - 1) // self.align * self.align
        closed = self.close() if self.end > self.first and self.used + a > self.budget else None
        self.end += 1
        self.used += a
        return closed

    def close(self):
        """Close the open group -> (first, end), or None when it is empty."""
        g = (self.first, self.end) if self.end > self.first else None
        self.first, self.used = self.end, 0
        return g

    def skip(self, n):
        """n sequences went another way (a padded batch); only with no group open."""
        assert self.end == self.first
        self.first = self.end = self.end + int(n)


def _cut_groups(lens, token_budget, align=8):
    """[(first, end)] of all groups of `lens` (any iterable, consumed lazily) through the streaming cutter."""
    cut, out = _GroupCutter(token_budget, align), []
    for n in lens:
        g = cut.add(n)
        if g is not None:
            out.append(g)
    g = cut.close()
    return out if g is None else out + [g]


class _TokenStage:
    """Pinned staging of the open group's token stream: two buffers that alternate, so the host fills one while the copy
    of the other is in flight (an event per buffer guards its reuse); they grow on demand."""

    def __init__(self, dev, capacity):
        self.dev = dev
        self.bufs = [torch.empty(max(int(capacity), 1024), dtype=torch.int32).pin_memory() for _ in range(2)]
        self.events = [None, None]
        self.cur = self.n = 0
        self.lens = []

    def push(self, tok):
        buf = self.bufs[self.cur]
        if self.n + len(tok) > buf.numel():
            grown = torch.empty(max(2 * buf.numel(), self.n + len(tok)), dtype=torch.int32).pin_memory()
            grown[:self.n] = buf[:self.n]
            buf = self.bufs[self.cur] = grown
        buf.numpy()[self.n:self.n + len(tok)] = tok
        self.n += len(tok)
        self.lens.append(len(tok))

    def upload(self):
        """-> (device int32 stream, host lens) of the staged group; staging moves on to the other buffer."""
        with torch.cuda.device(self.dev):
            tokens = self.bufs[self.cur][:self.n].to(self.dev, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
        self.events[self.cur] = ev
        lens = np.asarray(self.lens, np.int32)
        self.cur, self.n, self.lens = 1 - self.cur, 0, []
        if self.events[self.cur] is not None:
            self.events[self.cur].synchronize()       # (the copy before last: long done)
        return tokens, lens


def evaluate(args, eval_dataset, model, logger=None, token_budget=None):
    if token_budget is None:
        token_budget = getattr(args, "eval_token_budget", None)
    args.eval_batch_size = args.per_gpu_eval_batch_size * max(1, args.n_gpu)
    eval_sampler = SequentialSampler(eval_dataset)
    eval_dataloader = DataLoader(eval_dataset, sampler=eval_sampler, batch_size=args.eval_batch_size,
                                 collate_fn=eval_dataset.get_collate_fn(args, "inference"))
    if logger is not None:
        logger.info("***** Running evaluation *****")
        logger.info("  Num examples = %d", len(eval_dataset))
        logger.info("  Instantaneous batch size per GPU = %d", args.per_gpu_eval_batch_size)
    model.zero_grad()
    set_seed(args)  # the reference re-seeds here (:132-133)
    embedding, embedding2id, raw_sequences = [], [], []
    model.eval()
    import inspect
    fwd = (model.module if hasattr(model, "module") else model).forward
    takes_lens = "seq_lens" in inspect.signature(fwd).parameters      # (BiEncoder.forward has no such extension)
    stats = {"forwards": 0, "groups": [], "padded_batches": 0, "token_budget": None if token_budget is None else int(token_budget)}
    if token_budget is not None:
        if int(token_budget) < 1:
            raise ValueError("token_budget must be a positive number of packed rows (got %r)" % (token_budget,))
        _evaluate_coalesced(args, eval_dataloader, model, takes_lens, int(token_budget), embedding, embedding2id, raw_sequences, stats)
    else:
        for batch in eval_dataloader:
            qids = batch["qid"]
            ids, id_mask = (ele.to(args.device, non_blocking=True) for ele in [batch["concat_ids"], batch["concat_id_mask"]])
            with torch.no_grad():
                # the collate function right-pads (utils/util.py:163-185): the host knows the lengths, no device round trip
                lens = batch["concat_id_mask"].sum(1).numpy().astype(np.int32)
                embs = model(ids, id_mask, seq_lens=lens) if takes_lens else model(ids, id_mask)
            embedding.append(embs.detach())
            stats["groups"].append((len(embedding2id), len(embedding2id) + len(qids)))
            stats["forwards"] += 1
            embedding2id.extend(qids)
            raw_sequences.extend(batch["history_utterances"])
    global last_evaluate_stats
    last_evaluate_stats = stats
    if not embedding:
        return np.zeros((0, 768), np.float32), embedding2id, raw_sequences
    embedding = torch.cat(embedding, 0).cpu().numpy()
    from .train import check_status
    check_status(model)      # token ids outside the embedding table: IndexError like the reference's lookup (models.py:141)
    return embedding, embedding2id, raw_sequences


def _evaluate_coalesced(args, eval_dataloader, model, takes_lens, token_budget, embedding, embedding2id, raw_sequences, stats):
    """The budgeted walk of evaluate(): appends the groups' embeddings (device tensors, dataset order) to `embedding`."""
    ragged = getattr(model.module if hasattr(model, "module") else model, "query_emb_ragged", None)
    cutter = _GroupCutter(token_budget, align=8)
    stage = None

    def flush(group):
        if group is None:
            return
        tokens, lens = stage.upload()
        assert len(lens) == group[1] - group[0]
        with torch.no_grad():
            embedding.append(ragged(tokens, lens).detach())
        stats["groups"].append(group)
        stats["forwards"] += 1

    for batch in eval_dataloader:
        qids = batch["qid"]
        flat = _flatten_prefix_batch(batch["concat_ids"].numpy(), batch["concat_id_mask"].numpy()) if ragged is not None else None
        if flat is None:
            # a mask with holes (or a model without the ragged entry): the open group goes first, then today's padded call
            flush(cutter.close())
            ids, id_mask = (ele.to(args.device, non_blocking=True) for ele in [batch["concat_ids"], batch["concat_id_mask"]])
            with torch.no_grad():
                lens = batch["concat_id_mask"].sum(1).numpy().astype(np.int32)
                embs = model(ids, id_mask, seq_lens=lens) if takes_lens else model(ids, id_mask)
            embedding.append(embs.detach())
            cutter.skip(len(qids))
            stats["padded_batches"] += 1
            stats["forwards"] += 1
        else:
            tokens, lens = flat
            if stage is None:
                stage = _TokenStage(args.device, min(token_budget, 1 << 18))
            o = 0
            for n in lens.tolist():
                flush(cutter.add(n))
                stage.push(tokens[o:o + n])
                o += n
        embedding2id.extend(qids)
        raw_sequences.extend(batch["history_utterances"])
    flush(cutter.close())
