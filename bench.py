"""Headline benchmark: BLAKE2f compressions/s, witness fill + constraint eval, 2^18 batch of
12-round compressions per GPU (BASELINE.json configs[2]; configs[4] with --mix).

    python bench.py [--gpus N --steps K --warmup W]    (N > 1: starts its N ranks itself)
    python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N   (same, launched)
    ... bench.py --gpus 8 --global-batch 1048576                 (BASELINE configs[3])
    python bench.py --full ...       (also the legs reported beside the headline, see below)
    python bench.py --dump-outputs DIR ...   (the last timed step's outputs as DIR/*.npy)

A plain run sets up, warms up, times --steps steps and prints the line; everything measured
beside the headline (the other path, floors, CPU baseline, Fp export, prover columns, hasher;
N > 1: collectives alone, witness gathers, the config-4 leg) runs only with --full, and its
fields are null without it.

One step = witness fill + constraint eval of the whole per-GPU batch: --path fused (the
headline) runs b2f_fill_eval_dev (record kernel + the fused kernel that checks every tile as it
assigns it; the trace is written once and never read back), --path split runs b2f_fill_dev then
b2f_eval_dev; the other path is timed beside it as "other_path". Inputs and the trace stay
resident in HBM. N > 1: by default every rank runs its
own 2^18 batch (weak scaling); --global-batch G shards G instances over the ranks with the
row-balanced dist.plan_shards (strong scaling). Either way the step ends with one all_reduce of
the verdict counters and one RCCL all_gather of the h' outputs. The whole witness table is
reassembled on every rank (dist.gather_trace: one all-gather per column into the final
column-major buffers) where it fits in HBM, timed apart ("witness_gather"); at N = 8 a
BASELINE configs[3] leg (2^20 sharded, gather of the full 241 GB table) runs after the headline
unless --config4 0 (--config4-world picks the N it runs at, for rehearsals). Rank 0 prints one
JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "zk-odst_amd"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md, chip-level parameters)
# The prover columns are bound by 256-bit Montgomery products: tools/mulbench.hip measures the
# product b2f_field.h uses (one generated asm block per product, b2f_mont_asm.h, round 5) at up to
# 162 G products/s chip-wide in pasta Fp and 136 in BN254 Fr (profiles/r05m_mulbench.txt: the best
# of its chain counts and occupancies for the same code; the round-4 per-step form: 153 / 127).
# Products per row the lookup call executes (round 5's one-pass design, 4 rows per lane, 1,024-row
# look-back blocks): the z pass 5.5 per row in the lanes (den factor, suffix, lane total; num
# factor, prefix, Q; K and z) + ~2 per row in the block's scans and look-back, and lk_npart_kernel
# ~1.2 (the num factor's A part, its block product and reduction) = 8.7. The permutation leg
# counts its products per call from the circuit's copy cycles.
MULBENCH_GPS = {"pallas": 162.2, "bn254": 136.3}
LOOKUP_PRODUCTS_PER_ROW = 8.7
LOOKUP_MIN_PRODUCTS_PER_ROW = 6  # the algorithm's: num, den factors + a grand product's 4 (the roofline's)
# Where the prover-column legs' numbers were diagnosed: committed records of earlier runs
# (historical, not measured by this run; DESIGN.md §4-5 tells the story)
LOOKUP_EVIDENCE = {
    "history_ms_per_call": "1.16 (round 4: permute pass + gp passes) -> 1.29-1.31 (one pass, r05h) -> "
                           "1.12-1.15 (asm product, 4 rows per lane, r05m/n) -> 1.04-1.08 (block windows "
                           "instead of row searches, r05p) -> 1.00-1.02 (window loads up front, 4 waves, r05q/r)",
    "files": ["profiles/r05r_lk_pmc.txt", "profiles/r05r_lk_clock_w4.txt", "profiles/r05q_lookup_ab_block_w4.jsonl",
              "profiles/r05w_lookup_ab_nowait_diag.jsonl"],
}
PERM_EVIDENCE = {
    "history_ms_per_call": "3.05 (round 3) -> 2.58-2.60 (factors fused with the chunk pass, r04o) -> "
                           "2.15-2.19 (sigma as keygen, divsteps inversion, r05) -> 2.07-2.13 (asm product, r05m/s)",
    "files": ["profiles/r04a_pm_pmc.txt", "profiles/r05r_pm_pmc.txt", "profiles/r05m_perm_ab_comba.jsonl"],
}
# 1 in BN254 Fr Montgomery form (R mod r) as four little-endian int64 limbs
FR_ONE_MONT = [int.from_bytes((0x0e0a77c19a07df2f666ea36f7879462e36fc76959f60cd29ac96341c4ffffffb
                               >> (64 * i) & (2**64 - 1)).to_bytes(8, "little"), "little", signed=True)
               for i in range(4)]
ADVICE_COLS = 10
ROW_BYTES = 4 * (ADVICE_COLS + 1)  # 10 advice u32 + 1 fixed u32
INPUT_BYTES = 216
EXIT_EXTRAS_TIMEOUT = 3  # ExtrasWatchdog fired: headline printed, an extra leg hung


class ExtrasWatchdog:
    """After the headline of an N > 1 run: if the legs that follow (all collective) are not done
    within `timeout` seconds -- one rank failed where the others wait in a collective -- rank 0
    prints the headline's JSON line with "extras" marked timed out and every rank ends with
    exit code EXIT_EXTRAS_TIMEOUT: the headline is complete, but a hung collective is a real
    failure and a launcher or CI must see it (each rank runs its own timer, started at the same
    barrier). timeout 0: off."""

    def __init__(self, timeout, rank, headline, exit_fn=None, out=None):
        import threading

        self._lock = threading.Lock()
        self._done = False
        self._rank = rank
        self._headline = headline
        self._exit = exit_fn or os._exit
        self._out = out or sys.stdout
        self._timeout = timeout
        self._timer = None
        if timeout > 0:
            self._timer = threading.Timer(timeout, self._fire)
            self._timer.daemon = True
            self._timer.start()

    def _fire(self):
        with self._lock:
            if self._done:
                return
            self._done = True
            if self._rank == 0:
                line = self._headline()
                line["extras"] = {"error": "timed out after %g s; the headline fields are "
                                           "complete" % self._timeout}
                self._out.write(json.dumps(line) + "\n")
                self._out.flush()
        self._exit(EXIT_EXTRAS_TIMEOUT)

    def finish(self):
        """True if the caller prints the line (the watchdog did not fire)."""
        with self._lock:
            if self._done:
                return False
            self._done = True
        if self._timer is not None:
            self._timer.cancel()
        return True


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def host_cpus():
    """The host's CPUs as this process sees them: logical CPUs, physical cores (distinct
    (package, core) pairs of /proc/cpuinfo), the affinity mask, the cgroup CPU quota."""
    info = {"logical": os.cpu_count(), "affinity": len(os.sched_getaffinity(0))}
    cores = set()
    try:
        pkg = core = None
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                k, _, v = line.partition(":")
                k = k.strip()
                if k == "physical id":
                    pkg = v.strip()
                elif k == "core id":
                    core = v.strip()
                elif not k and pkg is not None:
                    cores.add((pkg, core))
                    pkg = core = None
        if pkg is not None:
            cores.add((pkg, core))
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    info["model"] = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    info["physical_cores"] = len(cores) or None
    try:
        with open("/sys/fs/cgroup/cpu.max") as fh:
            q, per = fh.read().split()
        info["cgroup_cpu_quota"] = None if q == "max" else round(int(q) / int(per), 2)
    except (OSError, ValueError):
        info["cgroup_cpu_quota"] = None
    return info


def cpu_baseline(rounds, mix, target_s, threads):
    """Time the CPU oracle (oracle/, a C port of the same fill + eval) on a bounded sample of
    the same workload: `threads` OpenMP threads (the box's CPU share for one GPU), then one
    thread (the per-core rate). Test infrastructure: the checker."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from b2f import synth

    flags = oracle.use_fastest_build()  # x86-64-v4 (AVX-512) where the host has it

    chunk = max(2048, 64 * threads)  # ~0.5 GB of trace per 2,048 instances: memory bounded

    def run(seed, n, nt):
        x = synth.batch(n, rounds=rounds, rounds_mix=mix, seed=seed)
        ox = np.frombuffer(x.tobytes(), dtype=oracle.INPUT_DTYPE).copy()
        t0 = time.perf_counter()
        adv, fixed, h_out, off = oracle.fill(ox, nthreads=nt)
        rep = oracle.evaluate(adv, fixed, off, nthreads=nt)
        dt = time.perf_counter() - t0
        assert rep["first_failure"] == 2**64 - 1
        return dt

    run(1, chunk, threads)  # warm the thread pool and the allocator
    n2, dt2, seed = 0, 0.0, 2
    while dt2 < target_s:
        dt2 += run(seed, chunk, threads)
        n2 += chunk
        seed += 1
    n1, dt1 = 0, 0.0
    while dt1 < max(1.0, target_s / 5):
        dt1 += run(1000 + n1, 128, 1)
        n1 += 128
    rate, single = n2 / dt2, n1 / dt1
    hc = host_cpus()
    eff = rate / (threads * single)
    out = {"value": round(rate, 1), "unit": "compressions/s", "cores": threads, "kind": "port",
           "build": "gcc " + flags,
           "single_thread": round(single, 1), "scaling_efficiency": round(eff, 3),
           "host_cpus": hc["logical"], "host": hc,
           "sample": "%d x %s-round compressions in chunks of %d, oracle fill + eval "
                     "(%.1f s timed, %d threads; 1 thread: %d in %.1f s)"
                     % (n2, "mixed" if mix else rounds, chunk, dt2, threads, n1, dt1)}
    if hc["physical_cores"]:
        # not measured: the per-thread rate times every physical core at the measured
        # efficiency (the box's CPU share is `threads`)
        out["projected_all_physical_cores"] = round(single * hc["physical_cores"] * eff, 1)
    return out


DUMP_H_ROWS = 1 << 18      # h' rows dumped at most (the 2^18 headline batch: all of them)
DUMP_TRACE_ROWS = 1 << 17  # trace rows sampled
DUMP_SEED = 0x5962be5d


def dump_outputs(path, batch, torch):
    """--dump-outputs: what the last timed step left in the batch's output buffers, the arrays a
    caller of fill_evaluate (or fill + evaluate) receives, as float64 .npy files (every value
    is a 32-bit word, so float64 holds it exactly; 64-bit words are split low word first):
      h_out.npy       [rows, 16]  h' of instances h_out_rows.npy (all of them up to 2^18, else a
                                  seeded sorted sample), 8 u64 as 16 u32 words
      report.npy      [42]        the eval report's 21 u64 counters as u32 words
      trace.npy       [11, S]     the 10 advice columns and the fixed column at the S seeded
                                  sample rows trace_rows.npy (sorted, below used_rows)
    The samples depend only on the batch's shape, so two builds run with the same arguments
    dump the same cells: 33.6 + 11.5 MB at the headline size."""
    os.makedirs(path, exist_ok=True)
    rng = np.random.default_rng(DUMP_SEED)
    dev = batch.advice.device

    def words(t):
        return t.contiguous().cpu().numpy().view(np.uint32).astype(np.float64)

    if batch.n <= DUMP_H_ROWS:
        inst = np.arange(batch.n, dtype=np.int64)
        h = batch.h_out
    else:
        inst = np.sort(rng.integers(0, batch.n, DUMP_H_ROWS, dtype=np.int64))
        h = batch.h_out[torch.from_numpy(inst).to(dev)]
    rows = np.sort(rng.integers(0, batch.used_rows, min(DUMP_TRACE_ROWS, batch.used_rows),
                                dtype=np.int64))
    idx = torch.from_numpy(rows).to(dev)
    trace = torch.cat([batch.advice[:, idx], batch.fixed[idx].unsqueeze(0)])
    np.save(os.path.join(path, "h_out.npy"), words(h))
    np.save(os.path.join(path, "h_out_rows.npy"), inst.astype(np.float64))
    np.save(os.path.join(path, "report.npy"), words(batch.report))
    np.save(os.path.join(path, "trace.npy"), words(trace))
    np.save(os.path.join(path, "trace_rows.npy"), rows.astype(np.float64))


def free_port():
    import socket

    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def spawn_ranks(n, argv, script=None, grace_s=30.0, poll_s=0.2):
    """`bench.py --gpus N` (N > 1) started without a launcher (no WORLD_SIZE in the
    environment): start N fresh child processes of this script, one per GPU, with the
    torch.distributed env:// variables set (RANK = LOCAL_RANK = k, WORLD_SIZE = N, master
    127.0.0.1 on a free port), and return the exit status to end with. The parent has made no
    GPU call (it runs before torch is imported). Children inherit stdout, so rank 0's one JSON
    line is the run's output. Once a child fails, the others get `grace_s` seconds to finish
    (a rank waiting in a collective on the failed one never would) and are then terminated.
    The status returned is the first failing child's (the root cause; a signal death as
    128 + signal), else 0."""
    import signal
    import subprocess

    script = script or os.path.abspath(__file__)
    port = free_port()
    procs = []

    def stop_all():
        for p in procs:
            if p.poll() is None:
                p.send_signal(signal.SIGTERM)
        t_kill = time.monotonic() + 10
        for p in procs:
            try:
                p.wait(max(0.1, t_kill - time.monotonic()))
            except subprocess.TimeoutExpired:
                p.kill()
                p.wait()

    class Stopped(Exception):
        pass

    def on_signal(signum, frame):
        raise Stopped(signum)

    # the parent stopped (a launcher's time limit, ^C): its ranks stop with it
    old = {sg: signal.signal(sg, on_signal) for sg in (signal.SIGTERM, signal.SIGINT)}
    first_bad, deadline = None, None
    try:
        for k in range(n):
            env = dict(os.environ)
            env.update({"RANK": str(k), "LOCAL_RANK": str(k), "WORLD_SIZE": str(n),
                        "LOCAL_WORLD_SIZE": str(n), "GROUP_RANK": "0", "MASTER_ADDR": "127.0.0.1",
                        "MASTER_PORT": str(port)})
            procs.append(subprocess.Popen([sys.executable, script] + list(argv), env=env))
        while True:
            codes = [p.poll() for p in procs]
            for c in codes:
                if c is not None and c != 0 and first_bad is None:
                    first_bad = 128 - c if c < 0 else c
                    deadline = time.monotonic() + grace_s
                    log("bench: a rank exited with status %d; the others get %g s" % (first_bad, grace_s))
            if all(c is not None for c in codes):
                break
            if deadline is not None and time.monotonic() > deadline:
                stop_all()
                break
            time.sleep(poll_s)
    except Stopped as e:
        stop_all()
        first_bad = first_bad or 128 + int(e.args[0])
    finally:
        for sg, h in old.items():
            signal.signal(sg, h)
    return first_bad or 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=1 << 18, help="instances per GPU (weak scaling)")
    ap.add_argument("--global-batch", type=int, default=0,
                    help="instances over all GPUs, row-balanced shards (strong scaling; "
                         "BASELINE configs[3] is 1048576 at 8 GPUs)")
    ap.add_argument("--rounds", type=int, default=12)
    ap.add_argument("--mix", action="store_true", help="rounds uniform in {1,4,12} (config 5)")
    ap.add_argument("--cpu-seconds", type=float, default=10.0)
    ap.add_argument("--cpu-threads", type=int, default=16,
                    help="oracle threads for the CPU baseline: the box's CPU share for one GPU")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--export-rows", type=int, default=1 << 25,
                    help="rows of the Fp export timed after the headline loop (0 = skip)")
    ap.add_argument("--path", choices=["split", "fused"], default="fused",
                    help="fused (the headline): b2f_fill_eval_dev, one kernel that checks each "
                         "tile as it assigns it; split: the fill kernel then the eval kernel")
    ap.add_argument("--lookup-circuits", type=int, default=64,
                    help="lookup-argument columns for this many 2^17-row circuits of the trace "
                         "(reported beside the headline; 0 skips)")
    ap.add_argument("--perm-k", type=int, default=22,
                    help="permutation-argument columns for one 2^k-row circuit of the trace "
                         "(reported beside the headline; 0 skips)")
    ap.add_argument("--hasher-messages", type=int, default=1 << 16,
                    help="multi-block BLAKE2b over the chip: this many 1 KiB messages "
                         "(reported beside the headline; 0 skips)")
    ap.add_argument("--witness-gather", type=int, default=1 << 13,
                    help="N > 1, weak scaling: instances per rank of a separate batch whose "
                         "whole witness table is all-gathered to every rank (timed apart; 0 "
                         "skips). With --global-batch the step's own trace is gathered if it fits")
    ap.add_argument("--config4", type=int, default=1 << 20,
                    help="N = --config4-world without --global-batch: after the headline, run "
                         "BASELINE configs[3] (this many instances sharded, full witness "
                         "gather); 0 skips")
    ap.add_argument("--config4-world", type=int, default=8,
                    help="world size at which the config-4 leg runs (8 = BASELINE configs[3]; "
                         "a smaller N with a small --config4 rehearses the same code)")
    ap.add_argument("--gather-cap-gb", type=float, default=0.0,
                    help="treat every rank as having at most this much free HBM when deciding "
                         "whether a witness gather fits (0 = the real free memory; rehearses "
                         "the skip branch)")
    ap.add_argument("--extras-timeout", type=float, default=600.0,
                    help="N > 1: seconds allowed for everything after the headline (collectives "
                         "timed alone, witness gathers, the config-4 leg); past it rank 0 prints "
                         "the headline line with the extras marked timed out and every rank exits "
                         "(0 = no limit)")
    ap.add_argument("--aux-steps", type=int, default=5,
                    help="steps of the other path timed after the headline loop (0 = skip)")
    ap.add_argument("--floor-reps", type=int, default=10,
                    help="interleaved reps of the floor variants and product kernels (0 = skip)")
    ap.add_argument("--traffic", default=os.path.join(ROOT, "profiles", "pmc_traffic.json"),
                    help="PMC-derived HBM bytes per launch (tools/pmc_traffic.py output)")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the legs reported beside it (CPU baseline, "
                         "floors, the other path, Fp export, lookup and permutation columns, "
                         "hasher; N > 1: collectives alone, witness gathers, the config-4 leg). "
                         "Without it their fields are null")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step left (h', the "
                         "report, a seeded sample of trace rows; rank 0's) as DIR/<name>.npy")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # no launcher: become the launcher (fresh children, nothing here touches the GPU)
        sys.exit(spawn_ranks(args.gpus, sys.argv[1:]))

    import torch
    import torch.distributed as dist

    import b2f
    from b2f import dist as bdist
    from b2f import synth

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log("warning: --gpus %d but WORLD_SIZE %d; using WORLD_SIZE" % (args.gpus, world))
    # rehearsal of the N > 1 code path on a one-GPU box (never for measurements): every rank
    # on cuda:0, collectives over gloo
    rehearse = os.environ.get("B2F_BENCH_REHEARSE") == "1"
    # the N > 1 code path (process group, collectives, witness gather) at any world size, here
    # for a one-rank RCCL run on a one-GPU box: the collectives are real RCCL calls on the device
    dist_on = world > 1 or os.environ.get("B2F_BENCH_FORCE_DIST") == "1"
    solo = not dist_on  # the one-GPU legs beside the headline
    if rehearse:
        local = 0
    torch.cuda.set_device(local)
    if dist_on:
        if rehearse:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
    device = "cuda:%d" % local
    mix = [1, 4, 12] if args.mix else None
    eng = b2f.Engine(local)
    stream = torch.cuda.current_stream().cuda_stream

    def make_batch(global_n):
        """This rank's batch: its own weak-scaling batch (global_n = 0) or its row-balanced
        shard of global_n instances. Returns (batch, shard info)."""
        if not global_n:
            n = args.batch
            x = synth.batch(n, rounds=args.rounds, rounds_mix=mix, first=rank * n)
            return b2f.DeviceBatch(x, device=device), {
                "rows": [0] * world, "base": 0, "window": None, "shards": None, "n_local": n}
        # shard plan from the rounds alone (synth's rounds depend only on the index)
        xr = synth.rounds_of(global_n, rounds=args.rounds, rounds_mix=mix)
        shards = bdist.plan_shards(xr, world)
        srows, sbase = bdist.shard_rows(xr, shards)
        w = bdist.trace_window(srows)
        lo, hi = shards[rank]
        x = synth.batch(hi - lo, rounds=args.rounds, rounds_mix=mix, first=lo)
        return b2f.DeviceBatch(x, device=device, total_rows=w), {
            "rows": srows, "base": sbase[rank], "window": w, "shards": shards,
            "n_local": hi - lo}

    def run_path(batch, path):
        if path == "fused":
            batch.fill_evaluate(eng, stream)
        else:
            batch.fill(eng, stream)
            batch.evaluate(eng, stream)

    def timed_loop(batch, info, path, steps, warmup, global_n):
        """Warm-up, then `steps` timed steps between barriers; returns (elapsed max over
        ranks, kernel times, verdict dict, h' gather buffer)."""
        gathered = verdict = None
        if dist_on:
            width = max(hi - lo for lo, hi in info["shards"]) if info["shards"] else info["n_local"]
            gathered = torch.empty((world * width, 8), dtype=torch.int64, device=device)
            hpad = torch.zeros((width, 8), dtype=torch.int64, device=device)

        def step():
            run_path(batch, path)
            nonlocal verdict
            if dist_on:
                verdict = bdist.all_reduce_verdict(
                    bdist.verdict_words(batch.report, info["base"], torch), dist)
                hsrc = batch.h_out
                if hsrc.shape[0] != hpad.shape[0]:
                    hpad[: hsrc.shape[0]].copy_(hsrc)
                    hsrc = hpad
                dist.all_gather_into_tensor(gathered, hsrc)

        for _ in range(warmup):
            step()
        eng.sync(stream)
        rep = batch.report_dict()
        if rep["first_failure"] != 2**64 - 1:
            raise SystemExit("eval flagged the trace: %s" % rep)
        eng.set_timing(True)
        if dist_on:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        torch.cuda.synchronize()
        if dist_on:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        ktimes = eng.kernel_times()
        eng.sync(stream)
        rep = batch.report_dict()
        if dist_on:
            t = torch.tensor([elapsed], dtype=torch.float64, device=device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
            v = verdict.tolist()
            if v[19] != bdist.NONE or sum(v[:19]) != 0:
                raise SystemExit("eval flagged a shard: %s" % v)
        if rep["first_failure"] != 2**64 - 1:
            raise SystemExit("eval flagged the trace: %s" % rep)
        return elapsed, ktimes, rep

    def collectives_alone(batch, info, steps):
        """The step's collectives timed alone (all-gather time apart)."""
        width = max(hi - lo for lo, hi in info["shards"]) if info["shards"] else info["n_local"]
        gathered = torch.empty((world * width, 8), dtype=torch.int64, device=device)
        hpad = torch.zeros((width, 8), dtype=torch.int64, device=device)
        hpad[: batch.n].copy_(batch.h_out)
        words = bdist.verdict_words(batch.report, info["base"], torch)
        dist.barrier()
        torch.cuda.synchronize()
        tc = time.perf_counter()
        for _ in range(steps):
            bdist.all_reduce_verdict(words, dist)
            dist.all_gather_into_tensor(gathered, hpad)
        torch.cuda.synchronize()
        ct = torch.tensor([time.perf_counter() - tc], dtype=torch.float64, device=device)
        dist.all_reduce(ct, op=dist.ReduceOp.MAX)
        return {"ms_per_step": round(1e3 * float(ct.item()) / steps, 4),
                "all_gather_bytes_per_rank": width * 64,
                "note": "2 all_reduce (verdict) + 1 all_gather (h'), timed alone"}

    def fits_everywhere(nbytes, margin=2 << 30):
        """True on every rank iff every rank has nbytes + margin of free HBM (collective)."""
        free = torch.cuda.mem_get_info(local)[0]
        if args.gather_cap_gb > 0:
            free = min(free, int(args.gather_cap_gb * 1e9))
        ok = torch.tensor([1 if free >= nbytes + margin else 0], dtype=torch.int64, device=device)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        return bool(ok.item()), free

    def witness_gather(adv, fixed, srows, x_note, reps=2):
        """Reassemble the whole witness table on every rank (gather_trace) and time it; the
        result is checked against the local shard (rank k's rows at its global offset)."""
        need = bdist.gather_trace_bytes(srows)
        ok, free = fits_everywhere(need)
        if not ok:
            return {"skipped": "needs %.1f GB per rank, %.1f GB free on rank %d"
                               % (need / 1e9, free / 1e9, rank)}
        buf = torch.empty((11, world * bdist.trace_window(srows)), dtype=adv.dtype, device=device)
        best = None
        for _ in range(reps):
            dist.barrier()
            torch.cuda.synchronize()
            tw = time.perf_counter()
            ga, gf = bdist.gather_trace(adv, fixed, srows, dist, torch, out=buf)
            torch.cuda.synchronize()
            wt = torch.tensor([time.perf_counter() - tw], dtype=torch.float64, device=device)
            dist.all_reduce(wt, op=dist.ReduceOp.MAX)
            best = float(wt.item()) if best is None else min(best, float(wt.item()))
        base = sum(srows[:rank])
        mine = srows[rank]
        same = bool(torch.equal(ga[:, base: base + mine], adv[:, :mine])) and \
            bool(torch.equal(gf[base: base + mine], fixed[:mine]))
        total = sum(srows)
        recv = (total - mine) * ROW_BYTES
        res = {"batch": x_note, "table_rows": total, "table_bytes": total * ROW_BYTES,
               "buffer_bytes_per_rank": need, "ms": round(best * 1e3, 3),
               "GBs_received_per_rank": round(recv / best / 1e9, 1),
               "own_rows_in_place": same,
               "note": "11 per-column all_gather_into_tensor into the final column-major "
                       "buffers (one RCCL group) + in-place compaction of padded windows"}
        del ga, gf, buf
        torch.cuda.empty_cache()
        return res

    global_n = args.global_batch
    batch, info = make_batch(global_n)
    n_local = batch.n
    rows = batch.used_rows
    log("rank %d: %d instances, %d rows, trace %.1f GB"
        % (rank, n_local, rows, batch.total_rows * ROW_BYTES / 1e9))

    total_n = global_n if global_n else world * n_local
    # the headline's config, captured once from the batch it times (later legs have their own
    # sizes and must not leak into it)
    if global_n:
        workload = ("%d x %s-round BLAKE2f compressions sharded over %d GPUs (row-balanced): "
                    "Table16 witness fill + constraint eval (LAYOUT v1)"
                    % (global_n, "{1,4,12}-mixed" if mix else args.rounds, world))
    else:
        workload = ("%d x %s-round BLAKE2f compressions per GPU: Table16 witness fill + "
                    "constraint eval (LAYOUT v1)"
                    % (n_local, "{1,4,12}-mixed" if mix else args.rounds))
    head_config = {"workload": workload, "batch_per_gpu": n_local, "global_batch": total_n,
                   "rounds": "mix{1,4,12}" if mix else args.rounds,
                   "rows_per_gpu": rows, "trace_bytes_per_gpu": rows * ROW_BYTES,
                   "path": args.path,
                   "parallelism": "dp%d (instance shards)" % world}

    elapsed, ktimes, rep = timed_loop(batch, info, args.path, args.steps, args.warmup, global_n)
    value = total_n * args.steps / elapsed
    ms_per_step = 1e3 * elapsed / args.steps
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, batch, torch)

    # roofline: algorithmic bytes per launch / average launch duration (HIP events)
    n = n_local
    fill_bytes = n * INPUT_BYTES + rows * ROW_BYTES      # inputs read + trace written
    eval_bytes = rows * ROW_BYTES + 8 * (n + 1)          # trace + offsets read

    def kernel_table(ktimes):
        kern = {}
        for name, nbytes in (("fill", fill_bytes), ("eval", eval_bytes),
                             ("fill_eval", fill_bytes), ("record", None)):
            tot, cnt = ktimes[name]
            if not cnt:
                continue
            avg = tot / cnt
            kern[name] = {"avg_ms": round(avg, 4), "launches": cnt}
            if nbytes:
                gbs = nbytes / (avg * 1e-3) / 1e9
                kern[name].update({"bytes_per_launch": nbytes, "achieved_GBs": round(gbs, 1),
                                   "frac": round(gbs / HBM_PEAK_GBS, 4)})
        return kern

    kern = kernel_table(ktimes)
    big = [k for k in kern if k != "record"]
    dom = max(big, key=lambda k: kern[k]["avg_ms"])
    # PMC traffic: only a record collected from these very kernel sources
    # counts -- the record carries the source stamp it was measured under (tools/pmc_traffic.py)
    traffic, traffic_src = None, None
    try:
        with open(args.traffic) as fh:
            tr = json.load(fh)
        key = "%s_%d_%s" % (dom, n, "mix" if mix else args.rounds)
        rec = tr.get(key, {})
        stamp = b2f._lib.source_stamp()
        if rec.get("source_stamp") == stamp:
            traffic = rec.get("hbm_bytes_per_launch")
            traffic_src = {"file": os.path.relpath(args.traffic, ROOT), "key": key,
                           "source_stamp": stamp, "kernels": rec.get("kernels")}
        else:
            traffic_src = {"file": os.path.relpath(args.traffic, ROOT), "key": key,
                           "stale": "recorded under sources %s, running %s" % (rec.get("source_stamp"), stamp)}
    except (OSError, ValueError):
        pass
    roof = {"bound": "hbm", "achieved": kern[dom]["achieved_GBs"], "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": kern[dom]["frac"], "traffic": traffic, "kernel": dom,
            "traffic_record": traffic_src}

    def headline():
        """The contract's fields of the JSON line, complete once the headline loop is done."""
        return {"metric": "BLAKE2f compressions/sec (witness+constraint eval), 2^18 batch, "
                          "1/2/4/8 GPU",
                "value": round(value, 1), "unit": "compressions/s", "n_gpus": world,
                "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 4),
                "higher_is_better": True, "scaling": "strong" if global_n else "weak",
                "vs_baseline": None, "dtype": "u32",
                "data": "synthetic (seeded splitmix64 h/m/t/f)",
                "config": dict(head_config),
                "roofline": roof, "cpu_baseline": None, "kernels": kern}

    # N > 1: the legs after the headline use collectives; one that hangs (a rank failing where
    # the others wait) must not cost the headline line, so a watchdog prints it and ends every
    # rank once the extras run past --extras-timeout (ExtrasWatchdog)
    watchdog = ExtrasWatchdog(args.extras_timeout if dist_on and args.full else 0, rank, headline)

    collectives = None
    witness = None
    if dist_on and args.full:
        collectives = collectives_alone(batch, info, args.steps)
        if global_n:
            witness = witness_gather(batch.advice, batch.fixed, info["rows"],
                                     "the step's own trace (%d instances)" % global_n)
        elif args.witness_gather > 0:
            try:
                nw = args.witness_gather
                xr = synth.rounds_of(world * nw, rounds=args.rounds, rounds_mix=mix)
                wshards = [(r * nw, (r + 1) * nw) for r in range(world)]
                wrows, _ = bdist.shard_rows(xr, wshards)
                xw = synth.batch(nw, rounds=args.rounds, rounds_mix=mix, first=rank * nw)
                wb = b2f.DeviceBatch(xw, device=device, total_rows=bdist.trace_window(wrows))
                wb.fill(eng, stream)
                eng.sync(stream)
                witness = witness_gather(wb.advice, wb.fixed, wrows,
                                         "a separate %d-instance batch per rank" % nw)
                del wb
            except Exception as e:
                witness = {"error": repr(e)}


    # same-box floors, from the diagnostics library (libb2f_diag.so; the product library has
    # no diagnostic variants): the fill with its stores but no cell computation
    # (B2F_DIAG_FILL=2), a plain store stream over the same columns (B2F_DIAG_FILL=4), the eval
    # with its loads, staging and lookups but no gates or copies (B2F_DIAG_EVAL=1; it fetches only
    # 0.86x the trace's bytes, so it is not a read floor) and a plain read stream over the same
    # columns (B2F_DIAG_EVAL=32, load_stream_kernel: the eval's read floor). Boxes differ by up to ~40 % in store rate, so the achieved/floor ratio
    # is the comparable number. Each rep launches floor and product kernels back to back
    # (fill floor, fused pass, split fill, eval floor, split eval), so drifts in the box's
    # store rate hit both sides alike; min and median over the reps are reported.
    floors = None
    if args.full and solo and args.floor_reps > 0:
        try:
            deng = b2f.Engine(local, diag=True)
            samples = {"fill_floor": [], "stream_floor": [], "fill_eval": [], "fill": [],
                       "eval_floor": [], "read_stream_floor": [], "eval": []}

            def one(e, fn, kname, var=None, val=None):
                if var:
                    os.environ[var] = val
                try:
                    e.set_timing(True)
                    fn(e, stream)
                    tot, cnt = e.kernel_times()[kname]
                finally:
                    if var:
                        os.environ.pop(var, None)
                return tot / max(cnt, 1)

            for _ in range(args.floor_reps):
                samples["fill_floor"].append(one(deng, batch.fill, "fill", "B2F_DIAG_FILL", "2"))
                samples["stream_floor"].append(one(deng, batch.fill, "fill", "B2F_DIAG_FILL", "4"))
                samples["fill_eval"].append(one(eng, batch.fill_evaluate, "fill_eval"))
                samples["fill"].append(one(eng, batch.fill, "fill"))
                samples["eval_floor"].append(one(deng, batch.evaluate, "eval", "B2F_DIAG_EVAL", "1"))
                samples["read_stream_floor"].append(one(deng, batch.evaluate, "eval", "B2F_DIAG_EVAL", "32"))
                samples["eval"].append(one(eng, batch.evaluate, "eval"))
            deng.sync(stream)
            deng.close()
            batch.fill(eng, stream)  # leave a real trace behind
            eng.sync(stream)
            med = {k: float(np.median(v)) for k, v in samples.items()}
            mn = {k: float(np.min(v)) for k, v in samples.items()}
            floors = {"reps": args.floor_reps, "interleaved": True,
                      "median_ms": {k: round(v, 4) for k, v in med.items()},
                      "min_ms": {k: round(v, 4) for k, v in mn.items()},
                      "max_ms": {k: round(float(np.max(v)), 4) for k, v in samples.items()},
                      "fill_floor_ms": round(med["fill_floor"], 4),
                      "eval_floor_ms": round(med["eval_floor"], 4),
                      "fill_over_floor": round(med["fill"] / med["fill_floor"], 4),
                      "eval_over_floor": round(med["eval"] / med["eval_floor"], 4),
                      "read_stream_floor_ms": round(med["read_stream_floor"], 4),
                      "eval_over_read_stream_floor": round(med["eval"] / med["read_stream_floor"], 4),
                      "fill_eval_over_fill_floor": round(med["fill_eval"] / med["fill_floor"], 4),
                      "fill_eval_over_fill_floor_min": round(mn["fill_eval"] / mn["fill_floor"], 4),
                      "stream_floor_ms": round(med["stream_floor"], 4),
                      "fill_eval_over_stream_floor": round(med["fill_eval"] / med["stream_floor"], 4),
                      "fill_eval_over_fill_min": round(mn["fill_eval"] / mn["fill"], 4),
                      "note": "ratios of medians (and of minima) over interleaved reps"}
        except (OSError, b2f.B2FError) as e:
            floors = {"error": repr(e)}

    # the other path, timed the same way (reported beside the headline, not part of it)
    aux = None
    other = "fused" if args.path == "split" else "split"
    if args.full and args.aux_steps > 0 and solo:
        run_path(batch, other)
        eng.sync(stream)
        eng.set_timing(True)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(args.aux_steps):
            run_path(batch, other)
        torch.cuda.synchronize()
        el = time.perf_counter() - t1
        k2 = kernel_table(eng.kernel_times())
        eng.sync(stream)
        r2 = batch.report_dict()
        aux = {"path": other, "value": round(n * args.aux_steps / el, 1),
               "ms_per_step": round(1e3 * el / args.aux_steps, 4), "kernels": k2,
               "verdict_clean": r2["first_failure"] == 2**64 - 1}

    # Fp export, reported beside the headline, not part of it:
    # Montgomery pallas limbs for a chunk of the resident trace (4 B read, 32 B written/cell)
    fp_export = None
    fp_export_bn254 = None
    if args.full and args.export_rows > 0 and solo:
        nr = min(args.export_rows, batch.total_rows)
        out = torch.empty((10, nr, 4), dtype=torch.int64, device=batch.advice.device)
        res = {}
        for form, name in ((b2f.FP_MONTGOMERY, "pasta Fp montgomery"),
                           (b2f.FP_BN254_MONTGOMERY, "bn254 Fr montgomery")):
            batch.export_fp(eng, nrows=nr, out=out, form=form, stream=stream)
            eng.sync(stream)
            eng.set_timing(True)
            reps = 5
            for _ in range(reps):
                batch.export_fp(eng, nrows=nr, out=out, form=form, stream=stream)
            tot, cnt = eng.kernel_times()["export"]
            avg = tot / max(cnt, 1)
            nbytes = nr * 10 * (4 + 32)
            res[form] = {"rows": nr, "form": name, "avg_ms": round(avg, 4),
                         "bytes_per_launch": nbytes,
                         "achieved_GBs": round(nbytes / (avg * 1e-3) / 1e9, 1),
                         "frac": round(nbytes / (avg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
        fp_export, fp_export_bn254 = res[b2f.FP_MONTGOMERY], res[b2f.FP_BN254_MONTGOMERY]
        del out

    # Lookup-argument prover columns for circuits cut from the resident
    # trace, and the multi-block hasher (row 3): reported beside the headline, not part of it
    lookup = None
    if args.full and solo and args.lookup_circuits > 0:
        try:
            usable = (1 << 17) - 7
            nc = min(args.lookup_circuits, batch.total_rows // usable)
            dev = batch.advice.device
            rb = torch.arange(nc, dtype=torch.int64, device=dev) * usable
            lout = torch.empty((nc, 5, usable + 1, 4), dtype=torch.int64, device=dev)
            lbad = torch.empty(nc, dtype=torch.int64, device=dev)
            chal = (0x1234567 << 200, 0x89ABCDEF << 180, 0x13579BDF << 190)

            def lk_call():
                eng.lookup_columns_dev(batch.advice.data_ptr(), batch.total_rows, rb.data_ptr(), nc,
                                       usable, *chal, 1, lout.data_ptr(), usable + 1,
                                       lbad.data_ptr(), stream)
            lk_call()
            eng.sync(stream)
            eng.set_timing(True)
            for _ in range(3):
                lk_call()
            tot, cnt = eng.kernel_times()["lookup"]
            avg = tot / max(cnt, 1)
            lrows = nc * usable
            # the roofline credits the algorithm's products (6 per row: the num and den
            # factors and the grand product's 4); the products the
            # implementation executes (its scans and look-back too) are a side field
            gps = lrows * LOOKUP_MIN_PRODUCTS_PER_ROW / (avg * 1e-3) / 1e9
            gps_exec = lrows * LOOKUP_PRODUCTS_PER_ROW / (avg * 1e-3) / 1e9
            lookup = {"circuits": nc, "usable_rows": usable, "avg_ms": round(avg, 4),
                      "rows_per_s": round(lrows / (avg * 1e-3)),
                      "algorithmic_GBs": round(lrows * 176 / (avg * 1e-3) / 1e9, 1),
                      "products_per_row": LOOKUP_MIN_PRODUCTS_PER_ROW,
                      "roofline": {"bound": "field products", "achieved": round(gps, 1),
                                   "peak": MULBENCH_GPS["pallas"], "unit": "G products/s",
                                   "frac": round(gps / MULBENCH_GPS["pallas"], 4),
                                   "executed_products_per_row": LOOKUP_PRODUCTS_PER_ROW,
                                   "executed_frac": round(gps_exec / MULBENCH_GPS["pallas"], 4)},
                      "field": "pasta Fp montgomery",
                      "all_rows_in_table": bool((lbad == -1).all().item()),
                      "evidence": LOOKUP_EVIDENCE}
            del lout
        except Exception as e:  # reported, never masks the headline
            lookup = {"error": repr(e)}
    # Permutation-argument prover columns of a 2^k-row circuit cut from
    # the resident trace: sigma (8 columns) + the grand products of ceil(8 / 3) column sets
    perm = None
    if args.full and solo and args.perm_k > 0:
        try:
            k = args.perm_k
            usable = (1 << k) - 7
            # the circuit holds the batch's first instances whose rows fit the usable rows
            # (selected by cumulative rows, so any rounds mix works)
            n_inst = int(np.searchsorted(batch.offsets_host[1:], usable, side="right"))
            n_inst = min(n_inst, batch.n)
            if n_inst == 0:
                raise ValueError("no instance fits 2^%d - 7 usable rows" % k)
            beta, gamma = 0x1234567 << 180, 0x89ABCDEF << 170
            form = b2f.FP_BN254_MONTGOMERY
            # keygen: sigma depends on the circuit's shape only, so a prover
            # computes it once (b2f_permutation_sigma_dev) and every proof's call writes z alone
            for _ in range(2):  # the first call builds the mapping pattern and its scratch
                eng.set_timing(True)
                sig = batch.permutation_sigma(eng, k, form=form, instances=(0, n_inst), stream=stream)
                sig_ms = eng.kernel_times()["perm_sigma"][0]
            z = None
            for rep in range(2):  # per-proof z calls: one untimed (scratch), then 3 timed
                eng.set_timing(True)
                for _ in range(1 if rep == 0 else 3):
                    _, z = batch.permutation_columns(eng, k, usable, beta, gamma, chunk_len=3,
                                                     form=form, instances=(0, n_inst),
                                                     sigma=False, stream=stream)
                tot, cnt = eng.kernel_times()["perm"]
            eng.sync(stream)
            avg = tot / max(cnt, 1)
            closes = bool(z[-1, usable].eq(torch.tensor(FR_ONE_MONT, dtype=torch.int64,
                                                        device=z.device)).all().item())
            domain = 1 << k
            # products the z call executes: per usable row 8 num coset values, 10 accumulations
            # (sets of 3, 3, 2 columns) and 4 per set of grand product, plus one den coset value
            # per cell on a copy cycle (the others map to themselves and reuse the num value),
            # summed over the instances' rounds; sigma (keygen) 8 per row of the 2^k domain
            on_cycle = 0
            from b2f import layout as blayout
            r_of = (np.diff(batch.offsets_host[:n_inst + 1].astype(np.int64))
                    - blayout.INIT_ROWS - blayout.FINAL_ROWS) // blayout.ROUND_ROWS
            for r, cnt_r in zip(*np.unique(r_of, return_counts=True)):
                mp = b2f.permutation_mapping(int(r))
                ident = ((mp >> 29) == np.arange(8, dtype=np.uint32)[:, None]) & \
                    ((mp & ((1 << 29) - 1)) == np.arange(mp.shape[1], dtype=np.uint32)[None, :])
                on_cycle += int((~ident).sum()) * int(cnt_r)
            products = usable * 30 + on_cycle
            gps = products / (avg * 1e-3) / 1e9
            perm = {"k": k, "instances": n_inst, "chunk_len": 3, "sets": 3,
                    "field": "bn254 Fr montgomery", "avg_ms": round(avg, 4),
                    "call": "per-proof z columns (sigma from keygen, below)",
                    "comparability": "from round 5 on the z call excludes sigma (keygen, timed "
                                     "apart as sigma_keygen); round <= 4 numbers included it",
                    "rows_per_s": round(domain / (avg * 1e-3)),
                    "products_per_row": round(products / domain, 2),
                    "roofline": {"bound": "field products", "achieved": round(gps, 1),
                                 "peak": MULBENCH_GPS["bn254"], "unit": "G products/s",
                                 "frac": round(gps / MULBENCH_GPS["bn254"], 4)},
                    "written_GBs": round(usable * 32 * 3 / (avg * 1e-3) / 1e9, 1),
                    "z_closes_to_one": closes,
                    "sigma_keygen": {"ms": round(sig_ms, 4), "products": domain * 8,
                                     "written_GBs": round(domain * 32 * 8 / (sig_ms * 1e-3) / 1e9, 1)},
                    "evidence": PERM_EVIDENCE}
            del sig, z
        except Exception as e:  # reported, never masks the headline
            perm = {"error": repr(e)}
    hasher_aux = None
    if args.full and solo and args.hasher_messages > 0:
        try:
            import hashlib

            from b2f import hasher
            hm = args.hasher_messages
            buf = np.random.default_rng(3).integers(0, 256, (hm, 1024), dtype=np.uint8)
            msgs = [bytes(r) for r in buf]
            plan = hasher.Plan(msgs)
            first = {}
            hasher.run_plan(eng, plan, phases=first)  # allocates the plan's workspace
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res = hasher.run_plan(eng, plan)  # reuses it: no allocation
            el2 = time.perf_counter() - t2
            phases = {}
            hasher.run_plan(eng, plan, phases=phases)  # again, phases timed apart (synchronizes)
            ok = res.verified and all(res.digests[i] == hashlib.blake2b(msgs[i]).digest()
                                      for i in range(0, hm, max(1, hm // 64)))
            hasher_aux = {"messages": hm, "bytes_each": 1024, "block_steps": plan.steps,
                          "compressions": int(plan.start[-1]), "ms": round(el2 * 1e3, 3),
                          "compressions_per_s": round(int(plan.start[-1]) / el2),
                          "digests_match_hashlib": ok,
                          "path": "fused",
                          "phases_ms": phases, "first_call_workspace_ms": first.get("workspace_ms"),
                          "note": "wall clock incl. block upload (one async copy from pinned "
                                  "memory) and the final h' download; the workspace made by the "
                                  "untimed first call is reused"}
        except Exception as e:
            hasher_aux = {"error": repr(e)}

    # BASELINE configs[3] after a weak-scaling headline at N = 8: 2^20 instances sharded over
    # the ranks, fill + eval timed the same way, then the whole witness table gathered
    # (--config4-world 2 --config4 32768 rehearses the same code on a one-GPU box)
    config4 = None
    if args.full and dist_on and world == args.config4_world and not global_n and args.config4 > 0:
        try:
            del batch
            torch.cuda.empty_cache()
            b4, i4 = make_batch(args.config4)
            el4, _, _ = timed_loop(b4, i4, args.path, args.steps, 1, args.config4)
            config4 = {"global_batch": args.config4, "rows_per_rank": i4["rows"],
                       "value": round(args.config4 * args.steps / el4, 1),
                       "ms_per_step": round(1e3 * el4 / args.steps, 4), "scaling": "strong",
                       "witness_gather": witness_gather(b4.advice, b4.fixed, i4["rows"],
                                                        "the step's own trace (%d instances)"
                                                        % args.config4, reps=1)}
            del b4
        except Exception as e:
            config4 = {"error": repr(e)}
        # free-memory evidence per rank for the 2^20 leg (the gather's buffers are the largest)
        if isinstance(config4, dict):
            config4["hbm_free_after_gb"] = round(torch.cuda.mem_get_info(local)[0] / 1e9, 1)

    cpu = None
    if args.full and rank == 0 and solo and not args.no_cpu:
        cpu = cpu_baseline(args.rounds, mix, args.cpu_seconds, args.cpu_threads)

    out = headline()
    out.update({"cpu_baseline": cpu, "floors": floors, "other_path": aux,
                "collectives": collectives, "witness_gather": witness, "config4": config4,
                "fp_export": fp_export, "fp_export_bn254": fp_export_bn254,
                "lookup_columns": lookup, "permutation_columns": perm, "hasher": hasher_aux,
                "gpu_vs_cpu": round(value / cpu["value"], 1) if cpu else None,
                "gpu_vs_cpu_threads": cpu["cores"] if cpu else None})
    if not watchdog.finish():
        return  # the watchdog printed the line and is ending the process
    if rank == 0:
        print(json.dumps(out), flush=True)
    if dist_on:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
