"""The reference's driver flow over block files (run_convdr_inference.py; the table in search.py's docstring), around whatever
index the caller hands in: a FlatIPIndex (device path) or any ``.add/.search/.reset`` object (host path)."""
import json
import os
import pickle

import numpy as np

from . import _lib
from .toplists import MAX_K, _check_max_depth, _distinct_row_depth, distinct_topk, distinct_topk_device, merge_topk, merge_topk_device


def load_block(path):
    """pickle.load, as run_convdr_inference.py:164-175 does."""
    with open(path, "rb") as h:
        return pickle.load(h)


def _check_distinct_certificate(who, counts, topN, m, rows_per_key, ann_data_dir, max_blocks, key_map):
    """The certificate of the ONE distinct step after a block walk at row depth m: a query with fewer than topN keys in m rows
    of a corpus that has more rows means rows_per_key was understated."""
    from . import blocks
    if (counts[:, 0] < 0).any():
        raise _lib.ConvdrError("%s: a record offset lies outside key_map (%d entries)" % (who, len(key_map)))
    open_ = np.nonzero((counts[:, 0] < topN) & (counts[:, 1] >= m))[0]
    if len(open_):
        most, total = blocks.key_row_stats(ann_data_dir, max_blocks, key_map)
        if total > m:
            raise _lib.ConvdrError("%s: %d queries hold fewer than %d keys in their top %d rows: "
                                   "rows_per_key = %d is understated (the id files give %d)"
                                   % (who, len(open_), topN, m, rows_per_key, most))


def search_distinct_one_by_one(ann_data_dir, gpu_index, query_embedding, topN, rows_per_key=None, key_map=None, max_blocks=8,
                               timings=None, max_depth=None):
    """``search_one_by_one`` at DOCUMENT level: per query the topN best distinct keys over all block files, each with the
    score and record offset of its best row -- what the reference gets from search_one_by_one + the `seen_pid` walk of
    EvalDevQuery (run_convdr_inference.py:58-69) only while the top-topN ROWS still hold topN documents.
    key: the record offset itself (key_map=None: MaxP blocks, where encode.py repeats the offset for every chunk row) or
    key_map[offset] (e.g. offset2pid, for a corpus with duplicate pids; numpy or torch int64).
    rows_per_key: the most rows any key owns (None: counted from the id files, blocks.max_rows_per_key).  The block walk
    runs ONCE, at row depth m = topN * rows_per_key <= FlatIPIndex.MAX_K -- deep enough for every query when rows_per_key
    is right -- the running merge is cut to m columns and ONE distinct step (device: convdr_topk_distinct) follows.  The
    certificate is checked: a query with fewer than topN keys in m rows of a corpus that has more rows means rows_per_key
    was understated -> ConvdrError; the walk is never silently repeated.
    Returns (D float64 [nq, topN], record offsets int64 [nq, topN]), the shapes EvalDevQuery reads; a corpus with fewer
    than topN keys leaves (-3.4028235e38, -1) in the tail.  Host path (an index without search_begin): every block needs
    at least m rows, as the reference's own id lookup does.
    max_depth (default FlatIPIndex.MAX_K, at most DEEP_MAX_K): the bound of m.  Beyond 4,096 the block searches are the deep
    ones, the running merge is merge_topk_sorted and the distinct step convdr_topk_distinct_deep."""
    from . import blocks
    max_depth = _check_max_depth("search_distinct_one_by_one", max_depth)
    topN = int(topN)
    if rows_per_key is None:
        rows_per_key = blocks.max_rows_per_key(ann_data_dir, max_blocks, key_map)
    rows_per_key = int(rows_per_key)
    m = _distinct_row_depth("search_distinct_one_by_one", topN, rows_per_key, max_depth,
                            "FlatIPIndex.MAX_K" if max_depth == MAX_K else "max_depth")
    merged = _search_block_list(ann_data_dir, gpu_index, query_embedding, m, range(max_blocks), True, timings)
    if merged is None:
        raise FileNotFoundError("no passage blocks under %s" % ann_data_dir)
    if hasattr(gpu_index, "search_begin"):
        import torch
        Dm, Im = merged[0][:, :m], merged[1][:, :m]
        km = key_map
        if km is not None:
            km = (km if torch.is_tensor(km) else torch.from_numpy(np.asarray(km, dtype=np.int64))).to(Dm.device, torch.int64)
        D, I, _, counts = distinct_topk_device(Dm, Im, topN, km)
        D, I, counts = D.double().cpu().numpy(), I.cpu().numpy(), counts.cpu().numpy()
    else:
        km = key_map.cpu().numpy() if hasattr(key_map, "cpu") else key_map
        D, I, _, counts = distinct_topk(merged[0][:, :m], merged[1][:, :m], topN, km)
    _check_distinct_certificate("search_distinct_one_by_one", counts, topN, m, rows_per_key, ann_data_dir, max_blocks, key_map)
    return D, I


def search_one_by_one(ann_data_dir, gpu_index, query_embedding, topN, max_blocks=8, timings=None):
    """Block-by-block search + merge; same contract as the reference function (float64 scores, int64 offsets,
    2 * topN columns once two blocks have been merged).  With a FlatIPIndex the embedding block is memory-mapped
    (blocks.BlockView: no pickle.load copy) and streamed to HBM in pinned chunks (FlatIPIndex.add), and the per-block
    results, the offset lookup ``embid[I]`` and the running merge stay on the device; any other index object
    (``.add/.search/.reset``) takes the reference's host path.
    Device path, pipelined: TWO blocks are in flight -- the first scan pass of block i is enqueued (search_begin, no host
    round trip), then the host reads block i + 1 into the twin index (file -> pinned staging -> HBM on the copy stream)
    while the GPU searches block i; block i's certificates are read (search_finish), its result merged and its storage
    dropped only after that.  The reference's load -> add -> search -> merge -> reset is strictly serial (:157-242).
    HBM residency: with two blocks in flight TWO fp32 blocks and their 16-bit scan copies are resident at once (2 x 1.5 x the
    block: 44 GB for CAsT's 14.6 GB blocks, of 288 GB) -- pass an index that is not a FlatIPIndex-with-twin, or search block
    files one at a time with index.add(BlockView) / search / reset yourself, where that does not fit.
    timings (optional dict): filled with the wall seconds spent per stage."""
    merged = _search_block_list(ann_data_dir, gpu_index, query_embedding, topN, range(max_blocks), True, timings)
    if merged is None:
        raise FileNotFoundError("no passage blocks under %s" % ann_data_dir)
    if hasattr(gpu_index, "search_begin"):
        return merged[0].double().cpu().numpy(), merged[1].cpu().numpy()
    return merged


def _search_block_list(ann_data_dir, gpu_index, query_embedding, topN, block_ids, stop_at_missing, timings=None):
    """The loop of ``search_one_by_one`` over the block files `block_ids`, in that order.  stop_at_missing: the first
    block whose embedding or id file cannot be read ends the walk (the reference's discovery, run_convdr_inference.py:
    159-177); otherwise (parallel.search_blocks_sharded: the ids of blocks that were found) such a block is an error.
    Returns the running merge as it stands -- device tensors (fp32, int64) on the device path, numpy (float64, int64) on
    the host path -- or None when no block was searched."""
    import time
    from . import blocks
    on_device = hasattr(gpu_index, "search_begin")
    merged = None
    tm = {"load_add_s": 0.0, "search_finish_merge_s": 0.0, "blocks": 0, "bytes": 0}

    def paths(block_id):
        return (os.path.join(ann_data_dir, "passage__emb_p__data_obj_%d.pb" % block_id),
                os.path.join(ann_data_dir, "passage__embid_p__data_obj_%d.pb" % block_id))
    if on_device:
        import torch
        twins = [gpu_index, None]
        pending = None                       # (handle, index, embid) of the block whose first pass is in flight

        def finish(p):
            nonlocal merged
            handle, idx, ids = p
            D, I = idx.search_finish(handle)
            embid = torch.as_tensor(np.asarray(ids, dtype=np.int64), device=D.device)
            found = torch.where(I >= 0, embid[I.clamp_min(0)], I) if embid.numel() else I   # -1 padding when n < topN
            cand = (D, found)
            merged = cand if merged is None else merge_topk_device(merged, cand, topN)
            idx.reset()
        for pos, block_id in enumerate(block_ids):
            emb_path, id_path = paths(block_id)
            try:
                view = blocks.BlockView(emb_path)
            except Exception:
                if stop_at_missing:
                    break
                raise
            try:
                try:
                    ids = load_block(id_path)
                except Exception:
                    if stop_at_missing:
                        break
                    raise
                idx = twins[pos & 1]
                if idx is None:
                    idx = twins[pos & 1] = gpu_index.twin()
                t0 = time.perf_counter()
                idx.add(view)                # the host reads; the GPU meanwhile searches the previous block
                t1 = time.perf_counter()
                tm["load_add_s"] += t1 - t0
                tm["bytes"] += int(view.array.nbytes)
                tm["blocks"] += 1
                if pending is not None:
                    finish(pending)
                pending = (idx.search_begin(query_embedding, topN), idx, ids)
                tm["search_finish_merge_s"] += time.perf_counter() - t1
            finally:
                view.close()                 # (streamed blocks: read by host threads that add() has joined; small blocks:
                                             #  copied synchronously by add() -- nothing reads the mapping any more)
        if pending is not None:
            t1 = time.perf_counter()
            finish(pending)
            tm["search_finish_merge_s"] += time.perf_counter() - t1
        if timings is not None:
            timings.update(tm)
        return merged
    for block_id in block_ids:
        emb_path, id_path = paths(block_id)
        try:
            passage_embedding = load_block(emb_path)
            passage_embedding2id = load_block(id_path)
        except Exception:
            if stop_at_missing:
                break
            raise
        gpu_index.add(passage_embedding)
        D, I = gpu_index.search(query_embedding, topN)
        cand = (D.astype(np.float64), np.asarray(passage_embedding2id)[I])
        merged = cand if merged is None else merge_topk(merged, cand, topN)
        gpu_index.reset()
    return merged


def EvalDevQuery(query_embedding2id, merged_D, dev_query_positive_id, I_nearest_neighbor, topN, output_file,
                 output_trec_file, offset2pid, raw_data_dir, output_query_type, raw_sequences=None,
                 load_collection=None):
    """Result writer with the reference's exact text output (run_convdr_inference.py:21-113).
    The offset -> pid mapping and the first-occurrence de-duplication (:56-69) run as array operations per query (one
    gather + one np.unique over the topN candidates) instead of the reference's Python loop over nq x topN entries."""
    ranked = {}
    raw = {}
    o2p = np.asarray(offset2pid)
    I_top = np.asarray(I_nearest_neighbor)[:, :topN]
    D_top = np.asarray(merged_D)[:, :topN]
    pids_all = o2p[I_top]                                   # offset -> pid for every candidate at once
    for query_idx in range(len(I_top)):
        query_id = query_embedding2id[query_idx]
        if query_id not in ranked:
            ranked[query_id] = [(0, 0)] * topN
        raw[query_id] = raw_sequences[query_idx]
        row = pids_all[query_idx]
        _, first = np.unique(row, return_index=True)        # first occurrence of every pid ...
        first.sort()                                        # ... in rank order
        scores = D_top[query_idx][first].tolist()
        for rank, (pid, score) in enumerate(zip(row[first].tolist(), scores)):
            ranked[query_id][rank] = (pid, score)
    queries = {}
    with open(os.path.join(raw_data_dir, "queries." + output_query_type + ".tsv")) as f:
        for line in f:
            qid, query = line.strip().split("\t")
            queries[qid] = query
    collection = os.path.join(raw_data_dir, "collection.jsonl")
    if not os.path.exists(collection):
        collection = os.path.join(raw_data_dir, "collection.tsv")
        if not os.path.exists(collection):
            raise FileNotFoundError("Neither collection.tsv nor collection.jsonl found in {}".format(raw_data_dir))
    all_passages = (load_collection or _load_collection)(collection)
    with open(output_file, "w") as f, open(output_trec_file, "w") as g:
        for qid, passages in ranked.items():
            for i in range(topN):
                pid, score = passages[i]
                label = 0 if qid not in dev_query_positive_id else dev_query_positive_id[qid].get(pid, 0)
                f.write(json.dumps({"query": queries[qid], "doc": all_passages[pid], "label": label,
                                    "query_id": str(qid), "doc_id": str(pid), "retrieval_score": score,
                                    "input": raw[qid]}) + "\n")
                g.write(str(qid) + " Q0 " + str(pid) + " " + str(i + 1) + " " + str(-i - 1 + 200) + " ance\n")


class _Passages(dict):
    def __missing__(self, key):
        return "[INVALID DOC ID]"


def _load_collection(collection_file):
    """utils/util.py:327-352 without the 50M-entry list: a dict with the same default."""
    all_passages = _Passages()
    ext = collection_file[collection_file.rfind(".") + 1:]
    if ext not in ["jsonl", "tsv"]:
        raise TypeError("Unrecognized file type")
    with open(collection_file) as f:
        for line in f:
            line = line.strip()
            if ext == "jsonl":
                obj = json.loads(line)
                all_passages[int(obj["id"])] = obj["title"] + "[SEP]" + obj["text"]
            else:
                try:
                    arr = line.split("\t")
                    all_passages[int(arr[0])] = arr[1].rstrip()
                except IndexError:
                    print("bad passage")
                except ValueError:
                    print("bad pid")
    return all_passages
