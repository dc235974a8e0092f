#!/usr/bin/env python3
"""bench.py -- ConvDR hot path on MI355X.  One JSON line on rank 0 (see the driver contract).

Workload = BASELINE.json configs[1]: "1 MI355X: 1M synthetic passages x 768-d encode + 1k-query brute-force IP
top-100, bf16 MFMA".  One step = one pass of the hot path over one batch:
  (i)   encode a batch of synthetic 128-token passages with the roberta-base-shaped rdot_nll encoder
        (random N(0, 0.02) weights, models.py:25-30) -> fp32 [batch, 768] embeddings,
  (ii)  append them to the block under construction (fp32 rows + bf16 scan copy + norm),
  (iii) run the exact 1k-query x 1M-passage inner-product top-100 search over the resident block.
`value` = passages encoded per second of whole-step time (search and fold included); the search rate is
reported beside it.  With N > 1 every rank owns a model replica and its own 1M-passage shard (weak scaling: the
corpus and the passage stream partition by rank).  The encode leg has no collective; the search leg has
the path's one real exchange step: the query embeddings are all-gathered, every rank searches its shard, the per-rank
top-k lists are all-gathered and merged on the device (parallel.search_sharded_device, BASELINE configs[3]).
A plain run sets up, warms up, times the steps and prints the line; --full adds what the line does not need (power state,
the roofline kernel under the profiler, the extra legs, the CPU baseline).  --dump-outputs DIR writes the last timed step's
embeddings and top-k (scores, ids) as .npy files; the inputs are seeded, so two builds can be compared output for output.
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0            # MI355X_MICROARCH.md: HBM3E 8 TB/s spec
MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense bf16 MFMA
H, I, LAYERS, HEADS, D_OUT = 768, 3072, 12, 12, 768
LINEAR_FLOP_PER_TOKEN = LAYERS * 2 * (4 * H * H + 2 * H * I)   # 169,869,312


def _rehearsal_device(local_rank):
    """CONVDR_BENCH_SHARE_GPU=1 (rehearsal on a 1-GPU box only): every rank uses cuda:0."""
    return 0 if os.environ.get("CONVDR_BENCH_SHARE_GPU") else local_rank


def _launch_ranks_if_needed(args):
    """`--gpus N` MEANS N ranks.  Called before anything touches the GPU (this process has imported neither torch nor the
    HIP library yet; a process that has initialised the GPU is never re-exec'd).
      * WORLD_SIZE set (torchrun / the driver's launch line) and == --gpus: this process is one of the ranks, go on.
      * WORLD_SIZE set and != --gpus: exit 2 -- a line labelled n_gpus = WORLD_SIZE under a `--gpus N` command is the
        worst failure mode a scaling run can have.
      * WORLD_SIZE unset and --gpus N > 1: this process becomes the launcher: N children of this same command line, one per
        device (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_ADDR = 127.0.0.1 / a free MASTER_PORT), rank 0's JSON line passes
        through on the inherited stdout, and the launcher exits with the first non-zero child status (the others are
        terminated) -- the one-process-per-GPU shape of gen_passage_embeddings.py:305-315 without needing torchrun."""
    ws = os.environ.get("WORLD_SIZE")
    if ws is not None:
        if int(ws) != args.gpus:
            sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%s: refusing to run a mislabelled job "
                             "(launch with --nproc-per-node == --gpus)\n" % (args.gpus, ws))
            sys.exit(2)
        return
    if args.gpus <= 1:
        return
    import socket
    import subprocess
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    kids = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), LOCAL_WORLD_SIZE=str(args.gpus),
                   MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
        kids.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    import signal

    def _stop(signum, frame):          # the launcher was told to stop: so are the ranks it started (exact PIDs, never a pattern)
        for k in kids:
            if k.poll() is None:
                k.terminate()
        sys.exit(128 + signum)
    for sig in (signal.SIGTERM, signal.SIGINT):
        signal.signal(sig, _stop)
    rc = 0
    live = set(range(args.gpus))
    while live:
        for r in sorted(live):
            st = kids[r].poll()
            if st is None:
                continue
            live.discard(r)
            if st != 0 and rc == 0:
                rc = st if st > 0 else 128 - st
                sys.stderr.write("bench.py launcher: rank %d exited with status %d; stopping the other ranks\n" % (r, st))
                for o in live:
                    kids[o].terminate()       # (exact PIDs this launcher started)
        time.sleep(0.05)
    sys.exit(rc)


def _init_group(dev):
    """RCCL ("nccl" on ROCm).  CONVDR_BENCH_BACKEND=gloo is the companion of CONVDR_BENCH_SHARE_GPU: RCCL refuses two ranks
    on one device, gloo moves the same CUDA tensors through the host -- the launch line, the rank logic and every kernel
    are the N > 1 run's, only the transport (and so the timing) is not."""
    import torch.distributed as dist
    backend = os.environ.get("CONVDR_BENCH_BACKEND", "nccl")
    if backend == "nccl":
        dist.init_process_group("nccl", device_id=dev)
    else:
        dist.init_process_group(backend)


def _comm_timed(fn, dev, reps=5):
    """ms per call of `fn` (a collective or a short chain around one): barrier, then `reps` calls between two events on the
    current stream, max over ranks."""
    import torch
    import torch.distributed as dist
    fn()
    torch.cuda.synchronize()
    dist.barrier()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    t = torch.tensor([a.elapsed_time(b) / reps], device=dev, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return t.item()


def _comm_common(dev, el):
    """What every N > 1 line says about its transport: the backend, the ranks the collective library really connected
    (an all-reduce of ones), and every rank's own clock around the timed region (min / max: a straggler shows here)."""
    import torch
    import torch.distributed as dist
    W = dist.get_world_size()
    ones = torch.ones(1, device=dev)
    dist.all_reduce(ones)
    els = [torch.zeros(1, device=dev, dtype=torch.float64) for _ in range(W)]
    dist.all_gather(els, torch.tensor([el], device=dev, dtype=torch.float64))
    els = [e.item() for e in els]
    return {"backend": dist.get_backend(), "world_size": W, "rccl_ranks_seen": int(round(ones.item())),
            "per_rank_elapsed_s": {"min": min(els), "max": max(els), "all": els},
            "shared_gpu_rehearsal": bool(os.environ.get("CONVDR_BENCH_SHARE_GPU"))}


def live_traffic(kname, timeout=240):
    """HBM-side bytes per launch of the roofline kernel measured IN THIS RUN: two child passes of this script (one step, no
    extras) under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (separate passes, counters only: MI355X_MICROARCH.md,
    HBM section), averaged over the kernel's dispatches.  None when rocprofv3 is not there or a pass fails."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        return None
    got = {}
    for ctr in ("FETCH_SIZE", "WRITE_SIZE"):
        td = tempfile.mkdtemp(prefix="convdr_pmc_")
        try:
            subprocess.run([exe, "--pmc", ctr, "--output-format", "csv", "-d", td, "--", sys.executable, os.path.join(ROOT, "bench.py"),
                            "--steps", "1", "--warmup", "0", "--passages", "65536", "--queries", "64", "--no-cpu-baseline", "--no-extras"],
                           cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=timeout, check=True)
            tot, cnt = 0.0, 0
            for path in glob.glob(os.path.join(td, "**", "*counter_collection.csv"), recursive=True):
                with open(path) as f:
                    for row in csv.DictReader(f):
                        if kname in row["Kernel_Name"] and row["Counter_Name"] == ctr:
                            tot += float(row["Counter_Value"])
                            cnt += 1
            if not cnt:
                return None
            got[ctr] = (tot / cnt, cnt)
        except Exception:
            return None
        finally:
            shutil.rmtree(td, ignore_errors=True)
    return got


def live_kernel_trace(kname, timeout=300):
    """Average dispatch duration (us) of the roofline kernel ON THE PROFILER'S CLOCK, measured in this run: one child pass
    of this script (4 steps after 2 warm-up steps, no extras) under `rocprofv3 --kernel-trace` -- the figure a reader
    reproduces with `rocprofv3 --kernel-trace --stats -- python bench.py` (profiles/rNN_bench_default.kernel_stats.txt).
    The first dispatches (warm-up) are dropped.  (avg_us, dispatches) or None."""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    exe = shutil.which("rocprofv3")
    if not exe:
        return None
    td = tempfile.mkdtemp(prefix="convdr_kt_")
    try:
        subprocess.run([exe, "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.join(ROOT, "bench.py"),
                        "--steps", "8", "--warmup", "4", "--passages", "65536", "--queries", "64", "--no-cpu-baseline", "--no-extras"],
                       cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                       timeout=timeout, check=True)
        rows = []
        for path in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    if kname in row["Kernel_Name"]:
                        rows.append((int(row["Start_Timestamp"]), int(row["End_Timestamp"])))
        rows.sort()
        rows = rows[len(rows) // 3:]                 # the warm-up steps' dispatches (4 of 12 steps; 4 + 2 until late in round 6: a
                                                     # 4-step pass read 0.400 where the next pass of the same command read 0.408)
        if not rows:
            return None
        return sum(e - b for b, e in rows) / len(rows) / 1e3, len(rows)
    except Exception:
        return None
    finally:
        shutil.rmtree(td, ignore_errors=True)


def _power_state():
    """What rocm-smi shows an ordinary user about the power state of device 0 (None when unreadable)."""
    import subprocess
    out = {}
    for flag, key in (("--showmaxpower", "max_power"), ("--showpower", "power"), ("--showclocks", "clocks")):
        try:
            r = subprocess.run(["rocm-smi", "-d", "0", flag, "--json"], capture_output=True, text=True, timeout=20)
            j = json.loads(r.stdout)
            out[key] = j.get("card0", j)
        except Exception:
            out[key] = None
    return out


def power_under_load(run_steps, seconds=2.5):
    """Socket power and shader clock WHILE the hot path runs (outside the timed region: `run_steps(n)` enqueues n more steps of the
    timed workload): rocm-smi polled from a thread for `seconds`.  MI355X's package cap is 1400 W; the MFMA kernels of this path
    sit at it (profiles/r05_power_probe.txt), which is what `clock_mhz_delivered` is the consequence of.  None when unreadable."""
    import re
    import subprocess
    import threading
    import torch
    samples, stop = [], threading.Event()

    def poll():
        while not stop.is_set():
            try:
                r = subprocess.run(["rocm-smi", "-d", "0", "--showpower", "--showclocks", "--json"], capture_output=True, text=True, timeout=10)
                c = json.loads(r.stdout).get("card0", {})
                w = [float(v) for k, v in c.items() if "power" in k.lower() and "max" not in k.lower()]
                f = [int(re.sub(r"\D", "", v)) for k, v in c.items() if k.lower().startswith("sclk clock speed")]
                if w and f:
                    samples.append((time.perf_counter(), w[0], f[0]))
            except Exception:
                return
            stop.wait(0.05)
    try:
        th = threading.Thread(target=poll, daemon=True)
        t0 = time.perf_counter()
        th.start()
        while time.perf_counter() - t0 < seconds:
            run_steps(4)
            torch.cuda.synchronize()
        stop.set()
        th.join(timeout=12)
        late = [(w, f) for t, w, f in samples if t - t0 > 0.4 * seconds]        # (rocm-smi's power figure is a moving average)
        if not late:
            return None
        ws, fs = sorted(w for w, _ in late), sorted(f for _, f in late)
        return {"socket_w_median": ws[len(ws) // 2], "socket_w_max": ws[-1], "sclk_mhz_median": fs[len(fs) // 2], "samples": len(late),
                "source": "rocm-smi --showpower --showclocks polled while %.1f s of extra steps of the timed workload run" % seconds}
    except Exception:
        stop.set()
        return None


def flop_per_passage(L):
    return LINEAR_FLOP_PER_TOKEN * L + 36864 * L * L + 2 * H * D_OUT


def random_rdot_model(seed=0):
    import contextlib
    import torch
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    torch.manual_seed(seed)
    # the model constructor announces "Using mean: ..." on stdout like the reference (models.py:134); stdout of this
    # script is reserved for the one JSON line
    with contextlib.redirect_stdout(sys.stderr):
        return MSMarcoConfigDict["rdot_nll"].model_class(RobertaConfig())


def synthetic_tokens(n, L, seed, device):
    import torch
    g = torch.Generator(device=device).manual_seed(seed)
    ids = torch.randint(3, 50000, (n, L), generator=g, device=device, dtype=torch.int32)
    ids[:, 0] = 0
    return ids


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy on the host; floating arrays keep float32 / float64, integer
    ones (top-k ids) become float64, which holds them exactly."""
    import numpy as np
    import torch
    os.makedirs(out_dir, exist_ok=True)
    for name, t in arrays.items():
        a = t.detach().float().cpu().numpy() if t.dtype in (torch.float16, torch.bfloat16) else t.detach().cpu().numpy()
        a = a.astype(np.float64 if a.dtype.kind in "iu" or a.dtype == np.float64 else np.float32)
        np.save(os.path.join(out_dir, name + ".npy"), a)


def cpu_baseline(nq, d, k, L, budget_s=9.0):
    """The reference's CPU path restated and timed on the host cores (bounded samples of the same workload):
    encode = the fp32 oracle forward (HF-free restatement of RobertaDot_NLL_LN.body_emb), search = exact fp32
    Q @ P.T + top-k (what FAISS-CPU IndexFlatIP computes; FAISS is not installed anywhere).
    `value` / `cores`: the run with min(64, available cores) threads.  BASELINE.md section 4 asks for
    torch.set_num_threads(os.cpu_count()); on the 256-thread bench host that run is 66x SLOWER (a 16-passage forward does
    not scale to 256 threads: 0.34 vs 22.6 passages/s in round 2), so it is reported beside the value, on a smaller
    sample to keep it bounded, instead of standing in for "what the CPU can do"."""
    import torch
    from oracle import encoder as OE
    avail = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    model = random_rdot_model()
    sd = {k_: v.detach() for k_, v in model.state_dict().items()}
    n = 50_000
    g = torch.Generator().manual_seed(0)
    P, Q = torch.randn(n, d, generator=g), torch.randn(nq, d, generator=g)

    def run(threads, B, budget, max_reps):
        torch.set_num_threads(threads)
        ids = synthetic_tokens(B, L, 0, "cpu").long()
        mask = torch.ones_like(ids)
        with torch.no_grad():
            t0, reps = time.perf_counter(), 0
            while reps < 1 or (time.perf_counter() - t0 < budget and reps < max_reps):
                OE.rdot_nll_emb(sd, ids, mask, num_layers=LAYERS, num_heads=HEADS)
                reps += 1
            enc_rate = B * reps / (time.perf_counter() - t0)
        t0, r2 = time.perf_counter(), 0
        while r2 < 1 or (time.perf_counter() - t0 < budget and r2 < 2 * max_reps):
            torch.topk(Q @ P.T, k, dim=1)
            r2 += 1
        return enc_rate, nq * n * r2 / (time.perf_counter() - t0), reps, r2
    # thread count: a short probe of 32 / 64 / 128 (VERDICT r05 "weak" 11: no intermediate counts were tried), the best one gets the
    # bounded timed sample; `cores` is "the best thread count tried", never "the host"
    cand = sorted({t for t in (32, 64, 128) if t <= avail} or {avail})
    probe = {}
    for t in cand:
        run(t, 2, 0.0, 1)                        # warm-up (thread pool, allocator)
        probe[t] = run(t, 16, 1.5, 3)[0]
    threads = max(probe, key=probe.get)
    enc_rate, ip_rate, reps, r2 = run(threads, 16, budget_s, 20)
    out = {"value": enc_rate, "unit": "passages/s", "cores": threads, "host_cores": os.cpu_count(), "available_cores": avail,
           "thread_probe_passages_per_s": {str(t): v for t, v in probe.items()},
           "kind": "port", "ip_pairs_per_s": ip_rate,
           "sample": "encode: 16 x %d-token passages x %d reps, fp32 torch oracle of RobertaDot_NLL_LN (12 x 768); "
                     "search: %d queries x %d passages x %d reps, fp32 SGEMM + topk(%d)" % (L, reps, nq, n, r2, k)}
    if avail > threads:
        e_all, i_all, _, _ = run(avail, 2, 0.0, 1)
        out["with_all_cores"] = {"value": e_all, "ip_pairs_per_s": i_all, "cores": avail,
                                 "sample": "encode: 2 passages x 1 rep; search: 1 rep (bounded: this configuration is far slower)"}
    return out


def train_kd_measure(dev, rank, world, dist_on, steps, warmup, Bt, with_kernels=True, dropout=0.1, teacher_cache=False):
    """configs[2]: run_convdr_train.py KD-only loop (MSE teacher-student), batch 64, seq 256, synthetic turns.
    dropout: hidden / attention-probability dropout of the student (the reference trains with model.train() and the
    released configs' 0.1, run_convdr_train.py:107); the teacher is in eval mode.
    teacher_cache: the frozen teacher's target embeddings come from a train.TeacherEmbeddingCache filled once before the timed
    region (what a second epoch, or a precompute pass, gives a real run) instead of a teacher forward per step -- numerically
    identical; NOT the reference flow, reported as its own leg.
    Returns the JSON-able result dict on rank 0 (None elsewhere); the caller owns the process group."""
    import numpy as np
    import torch
    import torch.distributed as dist
    from types import SimpleNamespace
    from convdr_amd import _lib, train as TR
    from convdr_amd.parallel import DataParallelStudent
    L_ = _lib.lib()
    Ls, Lt = 256, 64
    student = random_rdot_model(0).to(dev)
    teacher = random_rdot_model(0).to(dev).eval()
    student.config.hidden_dropout_prob = student.config.attention_probs_dropout_prob = float(dropout)
    TR.flatten_parameters(student)       # one fp32 arena: single-launch AdamW, single cast for the bf16 copies
    targs = SimpleNamespace(learning_rate=1e-5, adam_epsilon=1e-8, max_grad_norm=1.0, ranking_task=False, no_mse=False,
                            num_negatives=9, gradient_accumulation_steps=1)
    opt = TR.get_optimizer(targs, student, weight_decay=0.0)
    sched = TR.get_linear_schedule_with_warmup(opt, 0, 10_000)
    ddp = DataParallelStudent(student) if dist_on else None
    g = torch.Generator(device=dev).manual_seed(rank)

    def turns(L, lo):
        ids = torch.randint(3, 50000, (Bt, L), generator=g, device=dev)
        ids[:, 0] = 0
        lens = torch.randint(lo, L + 1, (Bt,), generator=g, device=dev)
        mask = (torch.arange(L, device=dev)[None, :] < lens[:, None]).long()
        return ids * mask, mask, lens.cpu().numpy().astype(np.int32)
    batches = []
    for _ in range(4):
        (ci, cm, cl), (ti, tm, tl) = turns(Ls, 32), turns(Lt, 8)
        # the collate function of a training loop knows the lengths on the host (it built the masks): handing them to
        # train_step removes the step's only device -> host round trip (CONVDR_BENCH_NO_HOST_LENS=1: the reference's
        # 4-tensor batch, lengths recovered from the device masks)
        batches.append((ci, cm, ti, tm) if os.environ.get("CONVDR_BENCH_NO_HOST_LENS") else (ci, cm, ti, tm, cl, tl))

    cache, sample_ids = None, [list(range(b * Bt, (b + 1) * Bt)) for b in range(4)]
    if teacher_cache:
        cache = TR.TeacherEmbeddingCache(4 * Bt, dim=D_OUT, device=dev)
        for b in range(4):
            kw = {} if len(batches[b]) < 6 else {"seq_lens": batches[b][5]}
            cache.fill(teacher, sample_ids[b], batches[b][2], batches[b][3], **kw)

    def step(i):
        kw = {"teacher_embs": cache.lookup(sample_ids[i % 4])} if cache is not None else {}
        return TR.train_step(targs, student, teacher, opt, sched, batches[i % 4], ddp=ddp, force_overlap=dist_on and world == 1, **kw)

    def sync_all():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
    # the step watchdog (train._StreamSets) probes its two stream sets on the first ~14 real steps of a process: done here,
    # before the warm-up, so that neither the W warm-up steps nor the K timed ones carry the probe
    # (N > 1: a fixed count -- every step holds collectives, so all ranks must run the same number of them)
    if dist_on:
        settle_steps = 16
        for i in range(settle_steps):
            step(i)
    else:
        settle_steps = TR.settle_streams(step, dev)
    gc.collect()
    gc.disable()          # (as in the headline loop: no cyclic-GC pause of the enqueuing host inside the timed region; in front of the warm-up)
    for i in range(warmup):
        step(i)
    sync_all()
    t0 = time.perf_counter()
    for i in range(steps):
        loss = step(i)[0]
    sync_all()
    el = time.perf_counter() - t0
    gc.enable()
    kern = {}
    if with_kernels:
        # per-kernel breakdown from a separate short pass: the hipEvent pair around each of the ~450 launches of a step
        # costs the host several milliseconds per step, which at this batch size would be the thing measured
        prof_steps = min(4, steps)
        L_.convdr_prof_enable(1)
        for i in range(prof_steps):
            step(i)
        sync_all()
        names = ("gemm_qkv", "gemm_attn_out", "gemm_ffn1", "gemm_ffn2", "gemm_dgrad", "gemm_wgrad", "attention", "attention_bwd",
                 "dgelu_colsum", "layernorm_bwd")
        for nme in names:
            ms, cnt = _lib.prof_collect(nme)
            if cnt:
                kern[nme] = {"ms_per_step": ms / prof_steps, "launches_per_step": cnt / prof_steps}
        L_.convdr_prof_enable(0)
    comm = None
    if dist_on:
        # ---- what the N > 1 line needs to explain itself (outside the timed region) ----
        comm = _comm_common(dev, el)
        # the gradient all-reduce that is NOT hidden under the backward: the same steps without the collectives (ddp = None:
        # every rank trains alone -- timing only, the replicas diverge from here on, which is why this comes last)
        sync_all()
        t1 = time.perf_counter()
        for i in range(steps):
            TR.train_step(targs, student, teacher, opt, sched, batches[i % 4])
        sync_all()
        el_no = time.perf_counter() - t1
        t2 = torch.tensor([el_no], device=dev, dtype=torch.float64)
        dist.all_reduce(t2, op=dist.ReduceOp.MAX)
        flat = student.roberta._flat["P"]
        bk = ddp._layer_buckets(flat.numel())
        comm["gradient_allreduce"] = {
            "exposed_ms_per_step": (el - t2.item()) / steps * 1e3,
            "ms_per_step_with": el / steps * 1e3, "ms_per_step_without_collectives": t2.item() / steps * 1e3,
            "path": getattr(ddp, "last_path", None),
            "collectives_per_step": (len(bk) + 2) if bk else 1,
            "bytes_per_layer_collective": int((bk[0][1] - bk[0][0]) * 4) if bk else None,
            "bytes_embeddings_collective": int(bk[0][0] * 4) if bk else None,
            "bytes_head_collective": int((flat.numel() - bk[-1][1]) * 4) if bk else None,
            "bytes_total_per_step": int(flat.numel() * 4)}
        big = torch.empty(flat.numel(), dtype=torch.float32, device=dev)
        comm["gradient_allreduce"]["one_collective_alone_ms"] = _comm_timed(lambda: dist.all_reduce(big), dev, reps=3)
        comm["gradient_allreduce"]["one_collective_alone_GB_per_s_algorithmic"] = flat.numel() * 4 / 1e9 / (comm["gradient_allreduce"]["one_collective_alone_ms"] / 1e3)
        comm["constructor_broadcast_collectives"] = ddp.broadcast_collectives
        del big
        # the same steps with the word-embedding gradient exchanged as (row ids, rows) -- DataParallelStudent(sparse_embedding=
        # True): one all-gather + a rank-ordered local scatter-add instead of the 154 MB dense all-reduce that cannot start
        # before the backward has ended.  Bytes of both forms per step and rank; the time is only meaningful over RCCL.
        ddp_s = DataParallelStudent(student, broadcast=False, sparse_embedding=True)
        for i in range(2):
            TR.train_step(targs, student, teacher, opt, sched, batches[i % 4], ddp=ddp_s, force_overlap=dist_on and world == 1)
        sync_all()
        t3 = time.perf_counter()
        for i in range(steps):
            TR.train_step(targs, student, teacher, opt, sched, batches[i % 4], ddp=ddp_s, force_overlap=dist_on and world == 1)
        sync_all()
        t3 = torch.tensor([time.perf_counter() - t3], device=dev, dtype=torch.float64)
        dist.all_reduce(t3, op=dist.ReduceOp.MAX)
        comm["gradient_allreduce"]["sparse_embedding_exchange"] = dict(
            ddp_s.last_comm, ms_per_step=t3.item() / steps * 1e3, exposed_ms_per_step=(t3.item() - t2.item()) / steps * 1e3,
            note="synthetic uniform token ids: ~8 k distinct ids among the ~9.2 k real tokens of a 64 x 256-token batch (the worst case; natural text repeats far more)")
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = t.item()
    if rank != 0:
        return None
    real_tokens = float(np.mean([b[1].sum().item() for b in batches]))   # (after the timed region)
    flop_dense = Bt * (3 * flop_per_passage(Ls) + flop_per_passage(Lt))
    flop_real = 3 * LINEAR_FLOP_PER_TOKEN * real_tokens
    sps = world * Bt * steps / el
    out = {
        "metric": "KD training samples/s (configs[2]: run_convdr_train.py KD-only, batch %d, seq %d/%d)" % (Bt, Ls, Lt),
        "value": sps, "unit": "samples/s", "n_gpus": world, "steps": steps, "warmup": warmup,
        "ms_per_step": el / steps * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "bf16 compute, fp32 master weights / optimizer", "data": "synthetic OR-QuAC-shaped turns (ragged)",
        "config": {"workload": "configs[2] train_kd" + (" with the frozen teacher's target embeddings looked up from a cache (not the reference flow)" if teacher_cache else ""),
                   "batch_per_gpu": Bt, "student_seq": Ls, "teacher_seq": Lt,
                   "parallelism": "dp%d" % world, "mean_real_student_tokens": real_tokens, "student_dropout": float(dropout)},
        "final_loss": float(loss),
        "stream_selfcheck": dict(TR.stream_decisions(dev), settle_steps=settle_steps),
        "comm": comm,
        "TFLOPs_dense_padded_count": sps / world * flop_dense / Bt / 1e12,
        "TFLOPs_real_token_count_linear_only": flop_real * steps / el / 1e12,
        "frac_of_bf16_mfma_peak_real_tokens": flop_real * steps / el / 1e12 / MFMA_BF16_PEAK_TFLOPS / world,
        "kernels": kern}
    del student, teacher, opt, batches
    torch.cuda.empty_cache()
    return out


def train_rank_measure(dev, Bt=64, K=10, Ld=512, steps=4, warmup=2):
    """configs[4]'s per-GPU step (run_convdr_train.py:101-193 with --ranking_task): B = 64 student turns of <= 256 tokens,
    teacher targets of <= 64, K = 10 documents x 512 tokens per sample.  Timed three ways: the reference's flow (the frozen
    teacher RE-ENCODES the 640 documents every step, :118-159), the lookup of the same embeddings from corpus blocks
    (`doc_embs=`), and the lookup with the all-gathered in-batch negatives of configs[4] (one rank here:
    the gather is the identity, the loss runs over B x K = 640 documents per query instead of 10)."""
    import numpy as np
    import torch
    from types import SimpleNamespace
    from convdr_amd import train as TR
    student = random_rdot_model(0).to(dev)
    teacher = random_rdot_model(1).to(dev).eval()
    student.config.hidden_dropout_prob = student.config.attention_probs_dropout_prob = 0.1
    TR.flatten_parameters(student)
    g = torch.Generator(device=dev).manual_seed(3)

    def turns(B, L, lo):
        ids = torch.randint(3, 50000, (B, L), generator=g, device=dev)
        ids[:, 0] = 0
        lens = torch.randint(lo, L + 1, (B,), generator=g, device=dev)
        mask = (torch.arange(L, device=dev)[None, :] < lens[:, None]).long()
        return ids * mask, mask, lens.cpu().numpy().astype(np.int32)
    (ci, cm, cl), (ti, tm, tl) = turns(Bt, 256, 32), turns(Bt, 64, 8)
    di, dm, _ = turns(Bt * K, Ld, Ld)                    # full 512-token documents
    batch = (ci, cm, ti, tm, cl, tl)
    with torch.no_grad():
        doc_embs = torch.cat([teacher(di[i:i + 128], dm[i:i + 128], is_query=False) for i in range(0, Bt * K, 128)], 0)
    out = {}
    for name, kw, inb in (("reencode_docs", {"doc_ids": di, "doc_mask": dm}, False), ("lookup_doc_embs", {"doc_embs": doc_embs}, False),
                          ("lookup_doc_embs_inbatch_negatives", {"doc_embs": doc_embs}, True)):
        targs = SimpleNamespace(learning_rate=1e-5, adam_epsilon=1e-8, max_grad_norm=1.0, ranking_task=True, no_mse=False,
                                num_negatives=K - 1, gradient_accumulation_steps=1, in_batch_negatives=inb)
        opt = TR.get_optimizer(targs, student, weight_decay=0.0)
        sched = TR.get_linear_schedule_with_warmup(opt, 0, 10_000)
        for i in range(warmup):
            TR.train_step(targs, student, teacher, opt, sched, batch, **kw)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(steps):
            loss, l1, l2 = TR.train_step(targs, student, teacher, opt, sched, batch, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / steps * 1e3
        out[name] = {"ms_per_step": ms, "samples_per_s": Bt / (ms / 1e3), "loss1_kd": float(l1.detach()), "loss2_rank": float(l2.detach())}
        del opt
    flop_docs = Bt * K * flop_per_passage(Ld)
    out["config"] = {"workload": "configs[4] per-GPU step: KD + ranking, batch %d, %d docs x %d tokens per sample" % (Bt, K, Ld),
                     "teacher_doc_TFLOP_per_step": flop_docs / 1e12, "student_dropout": 0.1}
    out["reencode_docs"]["teacher_doc_TFLOPs"] = flop_docs / 1e12 / ((out["reencode_docs"]["ms_per_step"] - out["lookup_doc_embs"]["ms_per_step"]) / 1e3)
    del student, teacher, doc_embs, di, dm
    torch.cuda.empty_cache()
    return out


def main_train(args):
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = _rehearsal_device(int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist_on = world > 1 or bool(os.environ.get("CONVDR_BENCH_FORCE_DIST"))   # (the latter: 1-rank rehearsal of the N > 1 path)
    if dist_on:
        _init_group(dev)
    out = train_kd_measure(dev, rank, world, dist_on, args.steps, args.warmup, args.train_batch, dropout=args.train_dropout,
                           teacher_cache=args.teacher_cache)
    if dist_on:
        dist.destroy_process_group()
    if out is not None:
        print(json.dumps(out))


def extras(dev, index, model, tower, head, building, filled_rows, nq, k, d, Q):
    """Legs reported beside the headline line (rank 0 of a 1-GPU run, outside the timed region)."""
    import shutil
    import tempfile
    import numpy as np
    import torch
    from convdr_amd import blocks
    from convdr_amd.search import FlatIPIndex
    out = {}
    # ---- (1) block file -> HBM: mmap'd pickle payload, pinned double-buffered chunks, bf16 preparation under the copy ----
    td = tempfile.mkdtemp(prefix="convdr_bench_")
    try:
        host = index._p32.cpu().numpy()
        path = os.path.join(td, "passage__emb_p__data_obj_0.pb")
        blocks.dump_block(path, host)
        del host
        rates = []
        for rep in range(3):                      # rep 0 also pins the (process-wide) staging buffers; the file is in the page cache
            with blocks.BlockView(path) as bv:
                fresh = FlatIPIndex(d, device=dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fresh.add(bv)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                rates.append(bv.array.nbytes / dt / 1e9)
                nb = bv.array.nbytes
                if rep == 2:
                    Dc, Ic = fresh.search_tensors(Q, k)
                    Dm, Im = index.search_tensors(Q, k)
                    same = bool((Ic == Im).all().item() and (Dc == Dm).all().item())
                del fresh
        # the ceiling of this box: pinned host memory -> HBM, nothing else (boxes of the pool differ: 44-57 GB/s)
        from convdr_amd.search import gpu_numa_cpus, pinned_near
        pin = pinned_near(dev, (1 << 28,), torch.uint8)     # on the GPU's NUMA node, like the loader's staging buffers
        dst = torch.empty_like(pin, device=dev)
        dst.copy_(pin, non_blocking=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(4):
            dst.copy_(pin, non_blocking=True)
        torch.cuda.synchronize()
        h2d = 4 * pin.numel() / (time.perf_counter() - t0) / 1e9
        del pin, dst
        out["block_load"] = {"GB_per_s": max(rates[1:]), "GB_per_s_first_call": rates[0], "GB_per_s_all_reps": rates, "bytes": nb,
                             "chunk_MB": 64, "pinned_h2d_ceiling_GB_per_s_this_box": h2d, "frac_of_h2d_ceiling": max(rates[1:]) / h2d,
                             "pcie_gen5_x16_GB_per_s": 63.0, "results_identical_to_resident_block": same,
                             "host_threads": len(os.sched_getaffinity(0)),
                             "gpu_numa_node_cpus": len(gpu_numa_cpus(dev) or ()) or None,
                             "path": "blocks.BlockView (payload offset of the pickle; page cache warm) -> positioned reads, 16 slices "
                                     "per chunk and 3 chunks in flight, into 4 process-wide pinned staging buffers -> H2D on a copy "
                                     "stream, convdr_ip_prepare_block_f16 of chunk i under the copy of chunk i + 1"}
        # ---- (1b) a-11 the way the reference runs it (run_convdr_inference.py:157-242): search_one_by_one over block FILES --
        # load -> add -> search -> merge -> reset per block, end to end, two blocks of 1M passages
        from convdr_amd.search import search_one_by_one
        host = index._p32.cpu().numpy()
        half = host.shape[0]
        for b in range(2):
            rows = host if b == 0 else np.ascontiguousarray(host[::-1])            # (second block: the same rows, reversed)
            blocks.dump_block(os.path.join(td, "passage__emb_p__data_obj_%d.pb" % b), rows)
            blocks.dump_block(os.path.join(td, "passage__embid_p__data_obj_%d.pb" % b), np.arange(b * half, (b + 1) * half, dtype=np.int64))
        del host
        Qh = Q.cpu().numpy()
        runs = []
        for rep in range(3):
            tmg = {}
            gi = FlatIPIndex(d, device=dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mD, mI = search_one_by_one(td, gi, Qh, k, timings=tmg)
            dt = time.perf_counter() - t0
            runs.append((dt, tmg))
            del gi
        dt, tmg = min(runs, key=lambda r: r[0])
        Dm, Im = index.search_tensors(Q, k)
        # every passage exists twice (row i of block 0 = row n - 1 - i of block 1), so the merged scores are the resident
        # block's top scores, each twice, and every returned offset folds back onto a row with exactly that score
        # (bit-exact ids against the oracle's search_one_by_one: tests/test_ip_search_gpu.py, tools/dbg/sobo_probe.py)
        want = Dm.double().cpu().numpy().repeat(2, axis=1)                    # the 2k merged entries: the resident top-k, twice
        fold = np.sort(np.where(mI < half, mI, 2 * half - 1 - mI), axis=1)
        rows_ok = bool((fold[:, 0::2] == fold[:, 1::2]).all() and (fold[:, 0::2] == np.sort(Im.cpu().numpy(), axis=1)).all())
        pair_ok = bool(mD.shape[1] == 2 * k and np.array_equal(mD, want) and rows_ok)
        out["search_one_by_one_files"] = {
            "blocks": 2, "passages_per_block": half, "queries": nq, "topk": k, "seconds_end_to_end": dt,
            "seconds_all_reps": [r[0] for r in runs], "file_GB_per_s_end_to_end": tmg["bytes"] / dt / 1e9,
            "breakdown_s": {"load_add (host: file -> pinned -> H2D enqueue, previous block's search running on the GPU)": tmg["load_add_s"],
                            "certify + merge + first pass enqueue": tmg["search_finish_merge_s"],
                            "queries H2D / result D2H / rest": dt - tmg["load_add_s"] - tmg["search_finish_merge_s"]},
            "merged_list_consistent_with_resident_search": pair_ok,
            "flow": "blocks.BlockView -> FlatIPIndex.add (streamed) -> search_begin; next block's add; search_finish -> convdr_topk_merge -> reset"}
    finally:
        shutil.rmtree(td, ignore_errors=True)
    out.update(extras_search(dev, index, tower, head, building, filled_rows, nq, k, d))
    return out


def extras_search(dev, index, tower, head, building, filled_rows, nq, k, d):
    import numpy as np
    import torch
    from convdr_amd.search import FlatIPIndex
    out = {}
    # ---- (2) search realism: what the encoder produces is clustered, which the N(0,1) corpus of the headline is not ----
    def timed_search(idx, Qx, reps=3):
        idx.search_tensors(Qx, k)                  # first search of the block: walks the precision ladder
        torch.cuda.synchronize()
        first = dict(idx.stats)
        t0 = time.perf_counter()
        for _ in range(reps):
            idx.search_tensors(Qx, k)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / reps * 1e3
        st = dict(idx.stats)
        return {"ms_per_search_incl_certify": ms, "pairs_per_s": Qx.shape[0] * idx.ntotal / (ms / 1e3),
                "queries_retried": st.get("retried"), "queries_on_split_bf16_scan": st.get("x3_queries"),
                "frac_on_split_bf16_scan": (st.get("x3_queries") or 0) / float(Qx.shape[0]), "kernel_rounds": st.get("rounds"),
                "started_on_split_bf16_scan": st.get("x3_first"), "first_search_of_block": first}
    g = torch.Generator(device=dev).manual_seed(7)
    n = index.ntotal
    c = torch.randn(d, device=dev, generator=g)
    Pc = 0.9 * c[None, :] + 0.12 * torch.randn(n, d, device=dev, generator=g)      # pairwise cosine ~ 0.98
    Qc = 0.9 * c[None, :] + 0.12 * torch.randn(nq, d, device=dev, generator=g)
    clustered = FlatIPIndex(d, device=dev)
    clustered.add(Pc)
    del Pc
    out["search_clustered"] = dict(timed_search(clustered, Qc), corpus="synthetic clustered: p = 0.9 c + 0.12 N(0,1), %d x %d" % (n, d))
    del clustered
    # the block the encoder wrote in the timed region (random-init roberta-base: LayerNorm'ed, strongly clustered outputs),
    # queries = freshly encoded token sequences
    with torch.no_grad():
        qtok = synthetic_tokens(min(nq, 1024), 32, 999, dev)
        Qe = tower.embed(qtok, None, head=head, seq_lens=np.full(qtok.shape[0], 32, np.int32))
    torch.cuda.empty_cache()
    # ---- (3) the same at the headline's size: 1M passages ENCODED by the model (489 batches of 2048 x 128 distinct
    # token sequences, ~25 s), 1k encoded queries: which rung certifies, and at what rate
    n_big = int(os.environ.get("CONVDR_BENCH_ENCODED_N", "1000000"))
    if n_big > 0:
        EB = 2048
        Pe = torch.empty((n_big, d), dtype=torch.float32, device=dev)
        lens = np.full(EB, 128, np.int32)
        t0 = time.perf_counter()
        with torch.no_grad():
            for s0 in range(0, n_big, EB):
                m = min(EB, n_big - s0)
                tok = synthetic_tokens(EB, 128, 5000 + s0 // EB, dev)
                Pe[s0:s0 + m] = tower.embed(tok, None, head=head, seq_lens=lens)[:m]
        torch.cuda.synchronize()
        enc_s = time.perf_counter() - t0
        big = FlatIPIndex(d, device=dev)
        big.add(Pe)
        res = timed_search(big, Qe)
        cnt = big.last_counts(Qe.shape[0], k)
        res.update(corpus="%d passages encoded by the random-init model (distinct 128-token sequences), %d encoded queries" % (n_big, Qe.shape[0]),
                   encode_s=enc_s, encode_passages_per_s=n_big / enc_s,
                   candidates_per_query={"emitted": cnt[0].float().mean().item(), "rescored_band": cnt[1].float().mean().item()})
        pw = torch.nn.functional.normalize(Pe[:4096] - Pe[:4096].mean(0, keepdim=True), dim=1)
        res["mean_pairwise_cosine_raw"] = float((torch.nn.functional.normalize(Pe[:2048], dim=1) @ torch.nn.functional.normalize(Pe[2048:4096], dim=1).T).mean())
        res["mean_abs_pairwise_cosine_centred"] = float((pw[:2048] @ pw[2048:].T).abs().mean())
        out["search_encoded_1m"] = res
        # a mid-size block of the same distribution (the two-best-of-64 threshold sample can only aim at rank n / 128 here:
        # expect one retry round)
        mid = FlatIPIndex(d, device=dev)
        mid.add(Pe[:47104].clone())
        out["search_encoded_47k"] = dict(timed_search(mid, Qe), corpus="the first 47,104 of those passages")
        del big, mid, Pe
        torch.cuda.empty_cache()
    return out


def extras_encode_loop(dev, model, n_pass=200_000, L=128):
    """a-8 end to end (gen_passage_embeddings.py:73-127): token cache ON DISK -> mmap reader -> token-budget batcher ->
    pinned staging -> encoder -> pinned fp32 block -> the two block files, ragged passages of 24..128 tokens."""
    import shutil
    import tempfile
    import numpy as np
    import torch
    from convdr_amd import blocks, encode
    rs = np.random.RandomState(0)
    lens = rs.randint(24, L + 1, size=n_pass)
    rec = np.zeros((n_pass, 4 + 4 * L), np.uint8)
    rec[:, :4] = np.stack([(lens >> s) & 255 for s in (24, 16, 8, 0)], 1).astype(np.uint8)
    ids = rs.randint(3, 50000, size=(n_pass, L)).astype(np.int32)
    ids[:, 0] = 0
    ids[np.arange(L)[None, :] >= lens[:, None]] = 0
    rec[:, 4:] = ids.view(np.uint8).reshape(n_pass, 4 * L)
    td = tempfile.mkdtemp(prefix="convdr_bench_enc_")
    try:
        base = os.path.join(td, "passages")
        rec.tofile(base)
        json.dump({"type": "int32", "total_number": n_pass, "embedding_size": L}, open(base + "_meta", "w"))
        del rec, ids
        with blocks.TokenCache(base) as cache:
            encode.encode_shard(model, cache, batch_size=8192, token_budget=262144, max_seq_length=L)    # warm-up pass
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            emb, embid = encode.encode_shard(model, cache, batch_size=8192, token_budget=262144, max_seq_length=L)
            t1 = time.perf_counter()
            blocks.dump_block(os.path.join(td, "passage__emb_p__data_obj_0.pb"), emb)
            blocks.dump_block(os.path.join(td, "passage__embid_p__data_obj_0.pb"), embid)
            t2 = time.perf_counter()
        return {"passages": n_pass, "real_tokens": int(lens.sum()), "lengths": "uniform 24..%d" % L,
                "passages_per_s": n_pass / (t1 - t0), "real_tokens_per_s": float(lens.sum()) / (t1 - t0),
                "passages_per_s_incl_block_write": n_pass / (t2 - t0), "block_write_s": t2 - t1,
                "path": "token cache file (page cache warm) -> blocks.TokenCache mmap -> encode.plan_batches (262,144 packed rows "
                        "per launch) -> pinned int32 staging -> encoder -> pinned fp32 block -> blocks.dump_block x 2"}
    finally:
        shutil.rmtree(td, ignore_errors=True)


def extras_registry(dev):
    """The rest of model.models.MSMarcoConfigDict (models.py:291-311) and the query-encode loop at the reference's own
    batch size: `dpr` (BiEncoder: two BERT-base towers, raw CLS, no head) and `rdot_nll_multi_chunk` (MaxP documents: one
    embedding per 512-token chunk) as encode rates, `evaluate` (run_convdr_inference.py:116-154) at per_gpu_eval_batch_size
    4 with conversational queries of up to 510 tokens as ms per batch -- small-batch latency of the persistent kernels."""
    import contextlib
    import logging
    from types import SimpleNamespace
    import numpy as np
    import torch
    from convdr_amd.inference import evaluate
    from convdr_amd.model.models import MSMarcoConfigDict, RobertaConfig
    out = {}

    def rate(fn, n_items, reps=5):
        with torch.no_grad():
            fn(); fn()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) / reps * 1e3
        return {"ms_per_batch": ms, "items_per_s": n_items / (ms / 1e3)}
    torch.manual_seed(0)
    with contextlib.redirect_stdout(sys.stderr):
        dpr = MSMarcoConfigDict["dpr"].model_class(SimpleNamespace()).to(dev).eval()
        mc = MSMarcoConfigDict["rdot_nll_multi_chunk"].model_class(RobertaConfig(max_position_embeddings=514)).to(dev).eval()
        rdot = random_rdot_model(0).to(dev).eval()
    g = torch.Generator(device=dev).manual_seed(11)

    def toks(B, L, vocab):
        ids = torch.randint(3, vocab, (B, L), generator=g, device=dev)
        ids[:, 0] = 0
        return ids
    ids, mask = toks(2048, 128, 30000), torch.ones(2048, 128, dtype=torch.long, device=dev)
    out["dpr"] = {"passages_2048x128": dict(rate(lambda: dpr(ids, mask, is_query=False), 2048), unit="passages/s (ctx_model, BERT-base)"),
                  "queries_64x32": dict(rate(lambda: dpr(ids[:64, :32], mask[:64, :32]), 64), unit="queries/s (question_model)")}
    ids_r = toks(2048, 128, 50000)
    out["rdot_nll_multi_chunk"] = {"passages_2048x128": dict(rate(lambda: mc(ids_r, mask, is_query=True), 2048), unit="sequences/s (query_emb path)")}
    dids, dmask = toks(64, 2048, 50000), torch.ones(64, 2048, dtype=torch.long, device=dev)
    dmask[:, 1536 + 100:] = 0        # the last chunk is partly padding, as after chunk-wise tokenisation
    out["rdot_nll_multi_chunk"]["docs_64x4x512"] = dict(rate(lambda: mc.body_emb(dids, dmask), 64, reps=3),
                                                        unit="documents/s (4 chunks of 512 tokens each, body_emb -> [64, 4, 768])")
    # evaluate(): CAsT-like sessions, right-padded to the batch maximum by the collate function
    rs = np.random.RandomState(5)
    nq, bs, Lq = 64, 4, 510
    lens = rs.randint(60, Lq + 1, size=nq)
    qids_np = rs.randint(3, 50000, size=(nq, Lq)).astype(np.int64)
    qids_np[:, 0] = 0
    qmask = (np.arange(Lq)[None, :] < lens[:, None]).astype(np.int64)
    qids_np *= qmask

    class DS(torch.utils.data.Dataset):
        def __len__(self):
            return nq

        def __getitem__(self, i):
            return i

        def get_collate_fn(self, args, mode):
            def collate(idx):
                m = int(lens[idx].max())
                return {"qid": ["q%d" % i for i in idx], "concat_ids": torch.from_numpy(qids_np[idx, :m]),
                        "concat_id_mask": torch.from_numpy(qmask[idx, :m]), "history_utterances": [[""] for _ in idx]}
            return collate
    eargs = SimpleNamespace(per_gpu_eval_batch_size=bs, n_gpu=1, device=dev, seed=42)
    log = logging.getLogger("bench")
    evaluate(eargs, DS(), rdot, log)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 3
    for _ in range(reps):
        emb, _, _ = evaluate(eargs, DS(), rdot, log)
    el = (time.perf_counter() - t0) / reps
    out["evaluate"] = {"queries": nq, "batch": bs, "max_tokens": Lq, "mean_tokens": float(lens.mean()),
                       "ms_per_batch": el / (nq / bs) * 1e3, "queries_per_s": nq / el,
                       "note": "whole evaluate() call incl. DataLoader, H2D of the batches and the final D2H (rdot_nll, batch 4)"}
    del dpr, mc, rdot
    torch.cuda.empty_cache()
    return out


def extras_search_38m(dev, nq, k, d):
    """BASELINE's target corpus on ONE MI355X: 38M x 768 resident (117 GB fp32 + 58 GB fp16 scan copy of 288 GB), built from
    8 slices of 4.75M generated on the device into reserved storage; 1k queries, top-100; and the HBM-bound regime at
    100 queries."""
    import torch
    from convdr_amd.search import FlatIPIndex
    free, total = torch.cuda.mem_get_info()
    n_slice, slices = 4_750_000, 8
    n = n_slice * slices
    if free < n * d * 6 + (20 << 30):
        return {"skipped": "only %.0f GB of HBM free" % (free / 1e9)}
    idx = FlatIPIndex(d, device=dev)
    idx.reserve(n)
    Q = torch.randn(nq, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    needles = torch.arange(nq, device=dev) * (n // nq) + 17
    t0 = time.perf_counter()
    for s in range(slices):
        P = torch.randn(n_slice, d, device=dev, generator=torch.Generator(device=dev).manual_seed(100 + s))
        sel = (needles >= s * n_slice) & (needles < (s + 1) * n_slice)
        P[needles[sel] - s * n_slice] = Q[sel]
        idx.add(P)
        del P
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0

    def timed(Qx, reps):
        D, I = idx.search_tensors(Qx, k)
        torch.cuda.synchronize()
        st = dict(idx.stats)
        t0 = time.perf_counter()
        for _ in range(reps):
            D, I = idx.search_tensors(Qx, k)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / reps * 1e3, st, D, I
    ms, st, D, I = timed(Q, 3)
    ok = bool((I[:, 0] == needles).all().item() and (D[:, :-1] >= D[:, 1:]).all().item())
    out = {"passages": n, "queries": nq, "topk": k, "build_s_8_slices_generated_on_device": build_s,
           "ms_per_search_incl_certify": ms, "pairs_per_s": nq * n / (ms / 1e3),
           "scan_TFLOPs_if_all_time_were_scan": 2.0 * nq * n * d / (ms / 1e3) / 1e12,
           "queries_retried": st.get("retried"), "rounds": st.get("rounds"), "planted_needles_rank_first_and_sorted": ok,
           "resident_GB": n * d * 6 / 1e9}
    ms100, st100, _, _ = timed(Q[:100].contiguous(), 3)
    out["nq100"] = {"ms_per_search": ms100, "pairs_per_s": 100 * n / (ms100 / 1e3),
                    "scan_copy_GB_per_s": n * d * 2 / (ms100 / 1e3) / 1e9, "frac_of_hbm_peak": n * d * 2 / (ms100 / 1e3) / 1e9 / HBM_PEAK_GBS,
                    "queries_retried": st100.get("retried")}
    del idx
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passages", type=int, default=1_000_000)
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--topk", type=int, default=100)
    ap.add_argument("--enc-batch", type=int, default=2048)
    ap.add_argument("--seq-len", type=int, default=128)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extras", action="store_true",
                    help="skip the legs reported beside the headline line: block file -> HBM load rate, search over "
                         "encoder-produced / clustered blocks, the configs[2] KD training step")
    ap.add_argument("--workload", default="encode_search", choices=["encode_search", "train_kd"],
                    help="encode_search = BASELINE configs[1] (the headline line); train_kd = configs[2]: KD-only "
                         "(MSE teacher-student) training steps, batch 64, student seq 256, teacher seq 64")
    ap.add_argument("--train-batch", type=int, default=64)
    ap.add_argument("--teacher-cache", action="store_true",
                    help="train_kd: the frozen teacher's target embeddings come from a train.TeacherEmbeddingCache (a second "
                         "epoch / precompute pass) instead of a teacher forward per step; not the reference flow")
    ap.add_argument("--train-dropout", type=float, default=0.1,
                    help="student dropout of the train_kd workload (the reference's training configuration: 0.1)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline line does not need: the power state, the roofline kernel under the "
                         "profiler (child passes), the extra legs (see --no-extras) and the CPU baseline (see --no-cpu-baseline)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step computed (embeddings, top-k scores and ids) "
                         "as DIR/<name>.npy in float32 / float64")
    args = ap.parse_args()
    _launch_ranks_if_needed(args)
    if os.environ.get("CONVDR_BENCH_LAUNCH_DRYRUN"):       # (tests/test_bench_launcher_cpu.py: the launcher without a GPU)
        print(json.dumps({k: os.environ.get(k) for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}), flush=True)
        sys.exit(int(os.environ.get("CONVDR_BENCH_LAUNCH_DRYRUN_FAIL_RANK", "-1")) == int(os.environ.get("RANK", "0")) and 7 or 0)
    if args.workload == "train_kd":
        return main_train(args)

    import numpy as np
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = _rehearsal_device(int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist_on = world > 1 or bool(os.environ.get("CONVDR_BENCH_FORCE_DIST"))   # (the latter: 1-rank rehearsal of the N > 1 path)
    if dist_on:
        _init_group(dev)
    from convdr_amd import _lib
    from convdr_amd.search import FlatIPIndex
    L_ = _lib.lib()
    if world == 1 and not dist_on and not args.no_extras:
        # (the train_kd / train_rank legs of --full: see train.reserve_streams; done without --full too, so that the timed
        #  steps' streams land on the same hardware queues either way)
        from convdr_amd import train as _TR
        _TR.reserve_streams(dev)

    n, nq, k, d, EB, SL = args.passages, args.queries, args.topk, D_OUT, args.enc_batch, args.seq_len
    model = random_rdot_model().to(dev).eval()
    tower, head = model.roberta, (model.embeddingHead, model.norm)
    pool = [synthetic_tokens(EB, SL, 100 * rank + i, dev) for i in range(4)]
    lens = np.full(EB, SL, np.int32)

    g = torch.Generator(device=dev).manual_seed(rank)
    P = torch.randn(n, d, device=dev, generator=g)
    Q = torch.randn(nq, d, device=dev, generator=torch.Generator(device=dev).manual_seed(1234))
    index = FlatIPIndex(d, device=dev)
    index.add(P)
    del P
    from convdr_amd import parallel
    embid = torch.arange(rank, rank + world * n, world, device=dev, dtype=torch.int64)   # records i % W == rank
    per = (nq + world - 1) // world
    Q_local = torch.zeros(per, d, device=dev)
    Q_local[:max(0, min(per, nq - rank * per))] = Q[rank * per:(rank + 1) * per]
    # freshly encoded embeddings go to the block under construction (searched once complete, like the reference's
    # encode-all-then-search flow); a ring of 32 batches stands in for it
    slots = 32
    building = FlatIPIndex(d, device=dev)
    building.add(torch.zeros(slots * EB, d, device=dev))
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
          for _ in range(args.steps)]

    retried = [0]
    last_emb = [None]

    def step(i, timers=None):
        with torch.no_grad():
            if timers:
                timers[0].record()
            emb = tower.embed(pool[i % len(pool)], None, head=head, seq_lens=lens)
            last_emb[0] = emb
            if timers:
                timers[1].record()
            building.update_rows((i % slots) * EB, emb)
            if dist_on:
                # configs[3]: every rank holds (has encoded) a slice of the queries -> all-gather of the query embeddings;
                # the corpus is sharded by block = rank: local exact top-k, two all-gathers, device merge
                Qall = parallel.all_gather_rows(Q_local, force=world == 1)[:nq]
                out = parallel.search_sharded_device(index, Qall, k, embid, force=world == 1)
            else:
                # the product path: FlatIPIndex.search_tensors = first pass + certification ladder for whatever the first
                # pass could not certify (nothing on this corpus: stats["retried"] is reported below)
                D_, I_ = index.search_tensors(Q, k)
                out = (D_, I_, None)
                retried[0] += index.stats.get("retried", 0)
            if timers:
                timers[2].record()
        return out

    def sync_all():
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()

    # the warm-up steps run exactly what the timed ones do, INCLUDING the instrumentation (hipEvent pairs around every launch, the
    # three timing events per step): the runtime creates its timestamp-signal pools on first use, and a one-off of that kind inside the
    # timed region is a 2-3 ms / step reading error at 20 steps (seen once in ~10 fresh-box runs: search + fold 4.4 instead of 1.8 ms)
    # (no cyclic-GC pass inside the timed region: the search's one host round trip per step makes every host pause a GPU stall, and a
    #  generation-2 collection of this process is tens of milliseconds.  Collected HERE, in front of the warm-up: a host pause directly in
    #  front of the timed steps lets the part drop its clocks, and the first timed kernels then run 20 % slow)
    gc.collect()
    gc.disable()
    L_.convdr_prof_enable(1)
    warm_ev = [tuple(torch.cuda.Event(enable_timing=True) for _ in range(3)) for _ in range(args.warmup)]
    for i in range(args.warmup):
        out = step(i, warm_ev[i])
    sync_all()
    del warm_ev
    # workgroup 0 of every FFN1 launch stamps {s_memtime, s_memrealtime} at its start and end: the shader clock the roofline
    # kernel actually ran at in this run (the part is power-managed; boxes of the pool differ by 4-5 % on identical code)
    n_probe = 512
    clock_probe = torch.zeros((n_probe, 4), dtype=torch.int64, device=dev)
    _lib.check(L_.convdr_set_option(b"clock_probe_slots", n_probe), "convdr_set_option")
    _lib.check(L_.convdr_set_option(b"clock_probe", clock_probe.data_ptr()), "convdr_set_option")
    L_.convdr_prof_enable(1)
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = step(i, ev[i])
    sync_all()
    el = time.perf_counter() - t0
    gc.enable()
    L_.convdr_set_option(b"clock_probe", 0)
    cp = clock_probe.cpu().numpy().astype(np.float64)
    cp = cp[cp[:, 3] > cp[:, 1]]                                 # the slots that were written (one per timed FFN1 launch)
    mhz = (cp[:, 2] - cp[:, 0]) / ((cp[:, 3] - cp[:, 1]) / 100.0) if len(cp) else np.zeros(0)      # s_memrealtime: 100 MHz
    clock_mhz = float(np.median(mhz)) if len(mhz) else None
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, {"embeddings": last_emb[0], "topk_scores": out[0], "topk_ids": out[1]})
    status_bad = int((out[2] != 0).sum().item()) if out[2] is not None else 0    # (after certification: always 0)
    first_pass_retries = retried[0]
    emitted, band = (t.float().mean().item() for t in index.last_counts(nq, k))
    enc_ms = sum(a.elapsed_time(b) for a, b, _ in ev) / args.steps
    ip_ms = sum(b.elapsed_time(c) for _, b, c in ev) / args.steps
    spans = {}
    for name in ("gemm_qkv", "gemm_attn_out", "gemm_ffn1", "gemm_ffn2", "attention", "layernorm", "embed_ln", "gemm_head",
                 "ip_scan_emit", "ip_scan_sample", "ip_rescore", "ip_cut", "ip_select", "ip_finish"):
        ms, cnt = _lib.prof_collect(name)
        if cnt:
            spans[name] = (ms / cnt, cnt, ms / args.steps)
    L_.convdr_prof_enable(0)
    comm = None
    if dist_on:
        # ---- what the N > 1 line needs to explain itself (outside the timed region): each exchange step timed on its own ----
        comm = _comm_common(dev, el)
        force = world == 1
        with torch.no_grad():
            Qall = parallel.all_gather_rows(Q_local, force=force)[:nq]
            Dl, Il = index.search_tensors(Qall, k)
            idl = embid[Il.clamp(min=0)]
            comm["query_allgather"] = {"ms": _comm_timed(lambda: parallel.all_gather_rows(Q_local, force=force), dev),
                                       "bytes_per_rank": int(Q_local.numel() * 4), "bytes_gathered": int(Q_local.numel() * 4 * world)}
            comm["topk_allgather_and_merge"] = {"ms": _comm_timed(lambda: parallel.exchange_topk(Dl, idl, k, force=force), dev),
                                                "bytes_per_rank": int(nq * k * 12), "bytes_gathered": int(nq * k * 12 * world),
                                                "merge_launches": world - 1}
            comm["local_certified_search_ms"] = _comm_timed(lambda: index.search_tensors(Qall, k), dev, reps=3)
        t = torch.tensor([el], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = t.item()
        dist.destroy_process_group()
    if rank != 0:
        return
    rows = EB * SL
    gemm_flop = {"gemm_qkv": 2.0 * rows * H * 3 * H, "gemm_attn_out": 2.0 * rows * H * H,
                 "gemm_ffn1": 2.0 * rows * H * I, "gemm_ffn2": 2.0 * rows * I * H,
                 "attention": 36864.0 / LAYERS * SL * SL * EB, "ip_scan_emit": 2.0 * nq * n * d}
    kern = {name: {"avg_ms": v[0], "launches": v[1], "ms_per_step": v[2],
                   **({"TFLOPs": gemm_flop[name] / v[0] / 1e9} if name in gemm_flop else {})}
            for name, v in spans.items()}
    dom = "gemm_ffn1"
    dom_tf = gemm_flop[dom] / spans[dom][0] / 1e9
    enc_rate = EB / (enc_ms / 1e3)
    line = {
        "metric": "passages encoded/sec + query x passage IP-scored/sec, 768-d",
        "value": world * EB * args.steps / el, "unit": "passages/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": el / args.steps * 1e3,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
        "data": "synthetic: uniform token ids in [3, 50000) with id[0] = 0, %d real tokens/passage; N(0,1) corpus/query "
                "embeddings (seed = rank / 1234); random-init roberta-base-shaped weights" % SL,
        "config": {"workload": "configs[1]: encode %d x %d-token passages per step into a resident %d x 768 block + "
                               "%d-query exact IP top-%d over the block" % (EB, SL, n, nq, k),
                   "passages_per_gpu": n, "queries": nq, "topk": k, "encode_batch": EB, "seq_len": SL,
                   "parallelism": "encoder replica + corpus shard (block = rank) per GPU x%d%s" % (
                       world, "; query embeddings all-gathered, per-rank top-k all-gathered and merged on device" if world > 1 else "")},
        "encode": {"passages_per_s_per_gpu": enc_rate, "ms_per_batch": enc_ms,
                   "TFLOPs_dense_count": enc_rate * flop_per_passage(SL) / 1e12,
                   "frac_of_bf16_mfma_peak": enc_rate * flop_per_passage(SL) / 1e12 / MFMA_BF16_PEAK_TFLOPS},
        "ip_search": {"pairs_per_s_per_gpu": nq * n / (ip_ms / 1e3), "ms_per_search_incl_fold": ip_ms,
                      "uncertified_queries": status_bad, "queries_retried_after_first_pass_all_steps": first_pass_retries,
                      "scan": "fp16 MFMA (v_mfma_f32_32x32x16_f16), eps = 1.07e-3 |q| max|p - centre|; certified by the fp64 re-score",
                      "candidates_per_query": {"emitted": emitted, "rescored_band": band}},
        "kernels": kern,
        "comm": comm,
        "roofline": {"kernel": "k_gemm<EPI_GELU_BLK> (FFN1 [%d x 768] x [768 x 3072], bias + GELU + blocked bf16 output fused)" % rows, "bound": "mfma",
                     "achieved": dom_tf, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s",
                     "frac": dom_tf / MFMA_BF16_PEAK_TFLOPS, "traffic": None},
    }
    # The same kernel on the profiler's clock, and its HBM-side traffic: from the committed rocprofv3 runs of this same
    # command (tools/dbg/refresh_profiles_r02.sh -> profiles/r02_*): --kernel-trace --stats for the average duration,
    # separate --pmc FETCH_SIZE / --pmc WRITE_SIZE passes for the traffic (FETCH_SIZE doubled per MI355X_MICROARCH.md
    # section HBM, counters in KB).  `achieved` / `frac` are measured live (hipEvents on the launch stream); the trace's
    # dispatch durations of back-to-back persistent GEMMs run 3-9 % longer, so both are stated.
    roof = line["roofline"]
    roof["achieved_hipevent"] = dom_tf
    if clock_mhz:
        # the same fraction against the matrix peak AT THE CLOCK THE KERNEL RAN AT (datasheet peak x delivered / 2400 MHz):
        # comparable across boxes and power states, where `frac` is not
        roof["clock_mhz_delivered"] = clock_mhz
        roof["clock_source"] = "s_memtime / s_memrealtime stamps of workgroup 0 of every timed FFN1 launch: median of %d" % len(mhz)
        roof["clock_mhz_min_max"] = [float(mhz.min()), float(mhz.max())]
        roof["peak_at_delivered_clock"] = MFMA_BF16_PEAK_TFLOPS * clock_mhz / 2400.0
        roof["frac_at_delivered_clock"] = dom_tf / roof["peak_at_delivered_clock"]
    roof["power"] = _power_state() if args.full and not args.no_extras else None     # (not in the profiler's child passes: rocm-smi is an exec)
    if args.full and not args.no_extras and not dist_on and roof["power"] is not None:
        roof["power_under_load"] = power_under_load(lambda n: [step(i) for i in range(n)])
    try:
        kname = "k_gemm<8, convdr::TileCfg<2, 4, 4, 2>"      # EPI_GELU_BLK on 256 x 256 tiles (k_gemm<1, ..> before round 3)
        rnd = next((r for r in ("r06", "r05", "r04", "r03", "r02") if os.path.exists(os.path.join(ROOT, "profiles", r + "_bench_default.kernel_stats.txt"))), "r02")
        if EB * SL == 262144:
            for ln in open(os.path.join(ROOT, "profiles", rnd + "_bench_default.kernel_stats.txt")):
                if kname in ln:
                    avg_us = float(ln[80:].split()[2])
                    roof["achieved_rocprof"] = gemm_flop[dom] / avg_us / 1e6
                    roof["frac_rocprof"] = roof["achieved_rocprof"] / MFMA_BF16_PEAK_TFLOPS
                    roof["rocprof_avg_us"] = avg_us
                    roof["rocprof_source"] = "profiles/%s_bench_default.kernel_stats.txt" % rnd
                    break
            pmc = json.load(open(os.path.join(ROOT, "profiles", rnd + "_pmc_hbm_traffic.json")))
            for kn, v in pmc.items():
                if kname in kn:
                    roof["traffic"] = (2.0 * v["FETCH_SIZE"] + v["WRITE_SIZE"]) * 1024.0
                    roof["traffic_source"] = "committed PMC run of this command (profiles/%s_pmc_hbm_traffic.json), NOT measured in this run" % rnd
                    roof["traffic_note"] = ("bytes per launch at the L2<->fabric boundary (Infinity-Cache hits included), "
                                            "profiles/%s_pmc_hbm_traffic.json; algorithmic bytes = %d"
                                            % (rnd, rows * H * 2 + rows * I * 2 + H * I * 2))
    except Exception:
        pass
    roof["frac_hipevent"] = roof["frac"]
    roof["frac_source"] = "hipEvent pairs on the launch stream around every timed FFN1 launch (no profiler pass in this run: it needs --full)"
    if args.full and world == 1 and not dist_on and not args.no_extras and EB * SL == 262144:
        # `achieved` / `frac` = the kernel's average dispatch duration on the PROFILER's clock, measured in this run by a child
        # pass under rocprofv3 --kernel-trace: the number `rocprofv3 --kernel-trace --stats -- python bench.py` reproduces
        # (profiles/r05_bench_default.kernel_stats.txt).  The hipEvent figure of the timed region stays beside it
        # (achieved_hipevent / frac_hipevent): back-to-back persistent GEMMs read 3-11 % longer under the tracer.
        kt = live_kernel_trace("k_gemm<8, convdr::TileCfg<2, 4, 4, 2>")
        if kt is not None:
            roof["rocprof_live_avg_us"], roof["rocprof_live_dispatches"] = kt
            roof["achieved"] = gemm_flop[dom] / kt[0] / 1e6
            roof["frac"] = roof["achieved"] / MFMA_BF16_PEAK_TFLOPS
            roof["frac_source"] = ("average dispatch duration of the kernel in a child pass of this script under rocprofv3 --kernel-trace "
                                   "(%d dispatches, measured in this run); hipEvent figure of the timed region: achieved_hipevent / frac_hipevent" % kt[1])
            if clock_mhz:
                roof["frac_at_delivered_clock_hipevent"] = roof["frac_at_delivered_clock"]
        # the roofline kernel's traffic, measured in this run (the committed PMC figure above stays beside it)
        lt = live_traffic("k_gemm<8, convdr::TileCfg<2, 4, 4, 2>")
        if lt is not None:
            if roof.get("traffic") is not None:
                roof["traffic_committed_run"] = roof["traffic"]
            roof["traffic"] = (2.0 * lt["FETCH_SIZE"][0] + lt["WRITE_SIZE"][0]) * 1024.0
            roof["traffic_source"] = ("measured in this run: child passes of this script under rocprofv3 --pmc FETCH_SIZE / --pmc WRITE_SIZE "
                                      "(separate passes, %d dispatches each); FETCH_SIZE doubled and both in KB per MI355X_MICROARCH.md" % lt["FETCH_SIZE"][1])
            roof["traffic_over_algorithmic"] = roof["traffic"] / float(rows * H * 2 + rows * I * 2 + H * I * 2)
    if args.full and world == 1 and not dist_on and not args.no_extras:
        try:
            line.update(extras(dev, index, model, tower, head, building, min(slots, args.steps + args.warmup) * EB, nq, k, d, Q))
            del index, building, model
            torch.cuda.empty_cache()
            keys = ("metric", "value", "unit", "ms_per_step", "steps", "warmup", "config", "final_loss", "TFLOPs_dense_padded_count",
                    "TFLOPs_real_token_count_linear_only", "frac_of_bf16_mfma_peak_real_tokens", "kernels", "stream_selfcheck")
            # (20 timed steps after 5 warm-up ones, like `--workload train_kd`: 10 / 3 read 0.0-0.2 ms higher than that line on the same box)
            kd = train_kd_measure(dev, 0, 1, False, 20, 5, 64, dropout=0.1)       # the reference's training configuration
            line["train_kd"] = {kk: kd[kk] for kk in keys}
            kd0 = train_kd_measure(dev, 0, 1, False, 20, 5, 64, with_kernels=False, dropout=0.0)
            line["train_kd_no_dropout"] = {kk: kd0[kk] for kk in ("value", "unit", "ms_per_step", "config", "final_loss")}
            kdc = train_kd_measure(dev, 0, 1, False, 20, 5, 64, with_kernels=False, dropout=0.1, teacher_cache=True)
            line["train_kd_teacher_cache"] = {kk: kdc[kk] for kk in ("value", "unit", "ms_per_step", "config", "final_loss")}
            line["train_rank"] = train_rank_measure(dev)
            line["encode_loop"] = extras_encode_loop(dev, random_rdot_model().to(dev).eval())
            line["registry"] = extras_registry(dev)
            torch.cuda.empty_cache()
            line["search_38m_1gpu"] = extras_search_38m(dev, nq, k, d)
        except Exception as e:      # the extras must never cost the headline line
            line["extras_error"] = "%s: %s" % (type(e).__name__, e)
    if args.full and not args.no_cpu_baseline:
        line["cpu_baseline"] = cpu_baseline(nq, d, k, SL)
    print(json.dumps(line))


if __name__ == "__main__":
    main()
