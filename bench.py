#!/usr/bin/env python3
"""
bench.py -- EI evaluations/second of the fused candidate sweep (+ GP-fit ms with --full).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c3|c5] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

A plain run sets up, runs W untimed and K timed steps and prints the line: `value`, `ms_per_step` (one
timed step) and the roofline of the timed kernels.  --full adds what takes work of its own: GP-fit ms,
the `configs` object and the CPU baseline (default config only).  --dump-outputs DIR writes what the
last timed step returned (rank 0's view) as float64 DIR/<name>.npy; the inputs are seeded, so two builds
run with the same arguments can be compared output for output.

Both launch forms work.  Called plainly with --gpus N > 1 the script starts N fresh rank
processes itself (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_PORT / IBO_COMM_ID_FILE in their
environment) BEFORE anything touches the GPU, relays rank 0's JSON line and exits non-zero if
any rank fails; under torch.distributed.run it reads the launcher's environment.  Either way
there is one process per GPU and no torch inside them (torch bundles its own HIP runtime; two
GPU runtimes in one process do not coexist): the RCCL unique id travels through a private file,
barriers and the max-over-ranks timing are RCCL collectives (ibo_amd/multigpu.py, csrc/comm.hip).

Default workload (BASELINE.json configs[1], SURVEY 8d "C2"): N=1024 observations, D=4,
squared-exponential ARD kernel theta=0.3, noise 0.1, X = RandomState(2).rand, Y =
sin(3 sum X)+0.01 randn; EI (xi=.01, libm erf, native clamp) over 2^20 candidates
per GPU = RandomState(102+rank).rand, already resident in HBM when the timed region
starts.  A "step" is one full sweep of the rank's candidates, ending with the
(best value, best index) on the host -- and, for N>1, the one RCCL arg-max
exchange.  Weak scaling: every rank sweeps its own 2^20 candidates (global M =
N * 2^20), the fitted GP is replicated (each rank fits it itself).

--config c3: BASELINE configs[2] as a strong-scaling sweep: N=2048, D=8, Matern-5/2, 4M
candidates cut into N contiguous shards, one EI sweep + one exchange per step.
--config c5: BASELINE configs[4]: N=4096, D=16, ARD marginal-likelihood grid, 64 theta-points
per GPU per step, gathered by one all-reduce (weak scaling; value = theta-points/s).

One JSON line on rank 0; `value` = all ranks' units * steps / max-over-ranks time.
roofline: the sweep kernel is fp64-MFMA bound; algorithmic flops per evaluation
F = N^2 + 3ND + 4N, achieved = F * M / mean kernel time measured with HIP
events on the kernel's own stream inside the timed region.
`configs` (--full, default config only, after the timed region): the other halves of the metric on
the same clock -- GP-fit ms at N=1024/2048/4096, the C3 shard sweep and gallery-8, the C4
preference GP (one GPU only) and the C5 grid, each with its own roofline block from SURVEY
8(d)'s flop counts.
cpu_baseline (--full, rank 0, N=1 only): the reference's own compiled C++ (oracle/_ref/libego.so,
negei through acqmaxGP with every dimension fixed = exactly one evaluation per call) on a
bounded sample of the same candidates; falls back to the plain-C port if _ref is absent.
"""
import argparse
import glob
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
T_START = time.perf_counter()

N_OBS, DIM, M_PER_GPU = 1024, 4, 1 << 20
FP64_PEAK_TFLOPS = 78.6          # MI355X fp64 matrix = vector peak (AMD spec; 256 CU x 4 SIMD x 32 flop/clk x 2.4 GHz)
C3_N, C3_D, C3_M_TOTAL, C3_SHARD = 2048, 8, 1 << 22, 1 << 19
C5_N, C5_D, C5_T = 4096, 16, 64


def f_eval(N, D):
    """algorithmic flops of one posterior + acquisition evaluation"""
    return N * N + 3 * N * D + 4 * N


def f_fit(N, D):
    """K assembly + Cholesky + W = L^-1 + alpha"""
    return N * N / 2.0 * (3 * D + 2) + 2.0 * N ** 3 / 3.0 + 2.0 * N * N


def f_nlml(N, D):
    """K assembly + Cholesky + the two reductions, no gradient"""
    return N * N / 2.0 * (3 * D + 2) + N ** 3 / 3.0 + 2.0 * N * N


def roofline_mfma(flops, seconds, **extra):
    a = flops / seconds / 1e12
    out = {"bound": "mfma", "achieved": a, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": a / FP64_PEAK_TFLOPS,
           "traffic": None}
    out.update(extra)
    return out


def dump_outputs(path, arrays):
    """--dump-outputs: one float64 .npy per array the last timed step returned"""
    if path is None:
        return
    os.makedirs(path, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), np.atleast_1d(np.asarray(a, dtype=np.float64)))


def synth(seed, N, D):
    rs = np.random.RandomState(seed)
    X = rs.rand(N, D)
    Y = np.sin(3 * X.sum(1)) + 0.01 * rs.randn(N)
    return X, Y


def hartman6(x):
    """ego/utils/testfunctions.py:280-304 (maximised), the C4 preference oracle"""
    A = np.array([[10, 3, 17, 3.5, 1.7, 8], [0.05, 10, 17, 0.1, 8, 14], [3, 3.5, 1.7, 10, 17, 8], [17, 8, 0.05, 10, 0.1, 14]])
    P = np.array([[0.1312, 0.1696, 0.5569, 0.0124, 0.8283, 0.5886], [0.2329, 0.4135, 0.8307, 0.3736, 0.1004, 0.9991],
                  [0.2348, 0.1451, 0.3522, 0.2883, 0.3047, 0.6650], [0.4047, 0.8828, 0.8732, 0.5743, 0.1091, 0.0381]])
    C = np.array([1, 1.2, 3, 3.2])
    return float(np.sum(C * np.exp(-np.sum(A * (x - P) ** 2, axis=1))))


def cpu_baseline(X, Y, cand, budget_s=3.0):
    """reference-shaped CPU evaluations/s on this host, 1 core (the reference is single-threaded)"""
    from oracle import oracle as orc
    ogp = orc.GP(orc.Kern("ard", [.3] * DIM), X, Y, noise=.1)
    invR = ogp.inv_factor()
    n = 0
    if orc.RefLib.available():
        ref = orc.RefLib()
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < budget_s and n < len(cand):
            q = cand[n]
            ref.acqmax(ogp, [[v, v] for v in q], orc.ACQ_EI, .01, maxiter=0, invR=invR)
            n += 1
        dt = time.perf_counter() - t0
        kind = "reference"
        what = "%d candidates through oracle/_ref/libego.so acqmaxGP (lb==ub, maxiter=0: one negei call each)" % n
    else:
        chunk = 256
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < budget_s and n < len(cand):
            orc.sweep_native(ogp, cand[n:n + chunk], orc.ACQ_EI, .01, invR=invR)
            n += chunk
        dt = time.perf_counter() - t0
        kind = "port"
        what = "%d candidates through oracle/ibo_oracle.c orc_sweep_native" % n
    out = {"value": n / dt, "unit": "EI evals/s", "cores": 1, "kind": kind, "sample": what}
    # what all host cores can do with the obvious algebra (alpha cached, triangular L^-1, OpenMP over
    # candidates): the plain-C port, ~1 s of work (the whole baseline stays within ~4 s of a default run)
    m = 2048
    t0 = time.perf_counter()
    r = orc.sweep_fast(ogp, cand[:m], orc.ACQ_EI, .01)
    dt = time.perf_counter() - t0
    while dt < 0.5 and m < len(cand):
        m = min(len(cand), m * 4)
        t0 = time.perf_counter()
        r = orc.sweep_fast(ogp, cand[:m], orc.ACQ_EI, .01)
        dt = time.perf_counter() - t0
    out["best_effort_all_cores"] = {"value": m / dt, "unit": "EI evals/s", "cores": r["threads"], "kind": "port",
                                    "sample": "%d candidates through oracle/ibo_oracle.c orc_sweep_fast (OpenMP)" % m}
    return out


# ------------------------------------------------------------------------------------------ launcher
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def self_launch(ngpus, argv, timeout_s=3000.0, script=None):
    """Start one fresh process per GPU and relay rank 0's JSON line.  Runs before this process has
    imported ibo_amd or made any HIP call: the children are ordinary subprocesses (never an exec of
    a process that touched the GPU).  Returns the exit status."""
    import shutil
    import tempfile
    rdv = tempfile.mkdtemp(prefix="ibo_bench_")              # 0700, fresh per run: nobody else can plant the id
    port = os.environ.get("MASTER_PORT") or str(_free_port())
    procs = []
    try:
        for r in range(ngpus):
            env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(ngpus), LOCAL_WORLD_SIZE=str(ngpus),
                       MASTER_ADDR="127.0.0.1", MASTER_PORT=port, IBO_COMM_ID_FILE=os.path.join(rdv, "rccl_id"),
                       IBO_BENCH_CHILD="1")
            env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
            # only rank 0 owns the JSON line; it goes to a file in the private directory, not a pipe: a line longer than the
            # pipe buffer would block rank 0 in write() while the launcher waits for it to exit
            out = open(os.path.join(rdv, "rank0.out"), "wb") if r == 0 else sys.stderr
            procs.append(subprocess.Popen([sys.executable, script or os.path.abspath(__file__)] + argv, env=env, stdout=out))
        t0 = time.time()
        status = 0
        pending = set(range(ngpus))
        while pending:
            for r in sorted(pending):
                rc = procs[r].poll()
                if rc is None:
                    continue
                pending.discard(r)
                if rc != 0 and status == 0:
                    status = rc if rc > 0 else 1
                    sys.stderr.write("bench.py: rank %d exited with status %d; stopping the other ranks\n" % (r, rc))
            if status != 0 or time.time() - t0 > timeout_s:
                if status == 0:
                    status = 4
                    sys.stderr.write("bench.py: ranks still running after %.0f s; stopping them\n" % timeout_s)
                for r in pending:
                    procs[r].terminate()                          # exactly the children started above
                for r in pending:
                    try:
                        procs[r].wait(20)
                    except subprocess.TimeoutExpired:
                        procs[r].kill()
                pending.clear()
                break
            if pending:
                time.sleep(0.05)
        with open(os.path.join(rdv, "rank0.out"), "rb") as f:
            line = f.read().decode("utf-8", "replace")
        if status == 0:
            sys.stdout.write(line)
            sys.stdout.flush()
            if not line.strip():
                sys.stderr.write("bench.py: rank 0 printed nothing\n")
                status = 5
        else:
            sys.stderr.write(line)
        return status
    finally:
        shutil.rmtree(rdv, ignore_errors=True)


# ------------------------------------------------------------------------------------------ worker
def pmc_numbers():
    """HBM bytes per launch cannot be read live; they come from committed rocprofv3 --pmc passes over this
    same command (tools/profile_bench.sh).  A summary is used only when it was taken from THIS build of the
    sweep kernel: its `source_sha` must equal the hash of the kernel sources in the tree."""
    h = hashlib.sha256()
    for f in ("ibo_amd/csrc/sweep2.hip", "ibo_amd/csrc/sweep.hip", "ibo_amd/csrc/ibo_common.h"):
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(fh.read())
    sha = h.hexdigest()[:16]
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_sweep_pmc.json")), reverse=True):
        try:
            j = json.load(open(p))
        except Exception:
            continue
        if j.get("source_sha") == sha:
            return j, os.path.relpath(p, ROOT), sha
    return None, None, sha


def config_pmc(name):
    """the committed PMC summary of a secondary roofline block (tools/profile_configs.sh -> profiles/r*_<name>_pmc.json), if it
    was taken from the kernel sources in the tree (tools/pmc_sources.json lists them per block); else (None, None, sha)"""
    try:
        files = json.load(open(os.path.join(ROOT, "tools", "pmc_sources.json")))[name]
    except Exception:
        return None, None, None
    h = hashlib.sha256()
    for f in files:
        with open(os.path.join(ROOT, f), "rb") as fh:
            h.update(fh.read())
    sha = h.hexdigest()[:16]
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_%s_pmc.json" % name)), reverse=True):
        try:
            j = json.load(open(p))
        except Exception:
            continue
        if j.get("source_sha") == sha:
            return j, os.path.relpath(p, ROOT), sha
    return None, None, sha


def attach_pmc(roofline, name, units=1.0):
    """fill `traffic` (HBM-side bytes: FETCH_SIZE x2 + WRITE_SIZE of the dominant kernel(s), per unit of the block) and the
    MFMA pipe utilisation from the committed summary, or say that none matches this build"""
    j, src, sha = config_pmc(name)
    roofline["kernel_source_sha"] = sha
    if j is not None and j.get("hbm_bytes_per_unit") is not None:
        roofline["traffic"] = j["hbm_bytes_per_unit"] * units
        roofline["traffic_kernels"] = j.get("kernels")
        roofline["traffic_source"] = "%s (rocprofv3 --pmc FETCH_SIZE x2, WRITE_SIZE; same kernel sources)" % src
        roofline["mfma_util_pct_pmc"] = j.get("mfma_util_pct")
        if j.get("valu_per_mfma") is not None:
            roofline["valu_per_mfma_pmc"] = j["valu_per_mfma"]
    else:
        roofline["traffic_source"] = "no committed PMC summary matches this build of the kernels"
    return roofline


def worker(args):
    # stdout carries exactly one line, the JSON: everything else that writes to file descriptor 1 (RCCL prints a
    # version / hostname / library-path banner through C stdio, flushed at exit) is sent to stderr
    sys.stdout.flush()
    json_fd = os.dup(1)
    os.dup2(2, 1)

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # IBO_BENCH_ONE_DEVICE=1: every rank on device 0, exchanges over ibo_amd.multigpu.SocketComm (RCCL refuses two ranks on one device).  A
    # CORRECTNESS run of the multi-rank path on a one-GPU box (tests/test_gpu_two_ranks.py) -- its numbers mean nothing: the ranks share the GPU.
    one_device = bool(os.environ.get("IBO_BENCH_ONE_DEVICE"))
    if one_device:
        local_rank = 0
    os.environ["IBO_DEVICE"] = str(local_rank)
    if world > 1:
        # one node: RCCL's bootstrap sockets go over loopback (the container hostname may not
        # resolve); the payload itself travels over xGMI peer-to-peer
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

    import ibo_amd                                                                  # noqa: F401
    from ibo_amd import _lib, DeviceArray
    from ibo_amd.gaussianprocess import GaussianProcess, PrefGaussianProcess
    from ibo_amd.gaussianprocess.kernel import GaussianKernel_ard, MaternKernel5
    from ibo_amd.gaussianprocess.trainhyper import nlml_grid
    from ibo_amd.acquisition import sweep
    from ibo_amd.acquisition.gallery import fastUCBGallery
    from ibo_amd.multigpu import RcclArgmax, exchange_unique_id, sharded_gallery, sharded_nlml_grid, shard_bounds

    _lib.check(_lib.lib.ibo_device_synchronize(local_rank))
    comm = None
    id_path = None
    if world > 1 or "RANK" in os.environ:          # launched as a rank (also with one rank)
        import threading

        def _stuck():
            sys.stderr.write("bench.py: RCCL communicator setup did not finish in 300 s (rank %d of %d)\n" % (rank, world))
            sys.stderr.flush()
            os._exit(3)
        watchdog = threading.Timer(300.0, _stuck)   # a rendezvous that never completes must not hang the node
        watchdog.daemon = True
        watchdog.start()
        if one_device:
            from ibo_amd.multigpu import SocketComm
            comm = SocketComm(world, rank, os.environ["IBO_COMM_ID_FILE"] + ".sock")
        else:
            uid, id_path = exchange_unique_id(world, rank)
            comm = RcclArgmax(world, rank, uid, device=local_rank)
        comm.barrier()
        watchdog.cancel()
        if comm.nranks() != world:
            raise SystemExit("RCCL reports %d ranks, expected %d" % (comm.nranks(), world))

    def barrier():
        _lib.check(_lib.lib.ibo_device_synchronize(local_rank))
        if comm is not None:
            comm.barrier()
        _lib.check(_lib.lib.ibo_device_synchronize(local_rank))

    def max_over_ranks(x):
        return x if comm is None else comm.argmax(x, rank)[0]

    def timed(step, steps, warmup):
        """W untimed steps, then exactly K steps between two barrier+synchronize pairs; max over ranks"""
        for _ in range(warmup):
            step()
        barrier()
        t0 = time.perf_counter()
        outs = [step() for _ in range(steps)]
        barrier()
        return max_over_ranks(time.perf_counter() - t0), outs

    base = {"n_gpus": world, "steps": args.steps, "warmup": args.warmup, "higher_is_better": True,
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "rccl_nranks": comm.nranks() if comm is not None else None,
            "transport": None if comm is None else ("socket, every rank on device 0 (a correctness run, not a measurement)" if one_device else "rccl"),
            "launcher": "self (bench.py children)" if os.environ.get("IBO_BENCH_CHILD") else
                        ("torch.distributed.run" if "RANK" in os.environ else "single process")}

    # ---------------------------------------------------------------- C3: strong-scaling sharded sweep
    def c3_setup(M_total):
        X, Y = synth(3, C3_N, C3_D)
        GP = GaussianProcess(MaternKernel5([.5, 1.0]), X, Y, noise=.1, device=local_rank)
        a, b = shard_bounds(M_total, world, rank)
        # every rank draws the same stream and keeps its own rows: the global array is the same for any N
        rs = np.random.RandomState(103)
        blk = 1 << 18
        rows = []
        for s0 in range(0, M_total, blk):
            chunk = rs.rand(min(blk, M_total - s0), C3_D)
            lo, hi = max(a, s0), min(b, s0 + len(chunk))
            if lo < hi:
                rows.append(chunk[lo - s0:hi - s0])
        host = np.concatenate(rows) if rows else np.zeros((0, C3_D))
        return GP, DeviceArray.from_host(host, local_rank), host, a

    def c3_step(GP, cand, host, start):
        if comm is None:
            r = sweep(GP, cand, acq='ei', xi=.01, native=True, index_base=start)
            return r["best_val"], r["best_idx"], r["kernel_ms"], r["kernel"]
        if getattr(comm, "device_exchange", False):       # RCCL: sweep + exchange in one device-side call (ibo_acq_sweep_exchange)
            r = sweep(GP, cand, acq='ei', xi=.01, native=True, index_base=start, exchange=comm)
            return r["global_val"], r["global_idx"], r["kernel_ms"], r["kernel"]
        r = sweep(GP, cand, acq='ei', xi=.01, native=True, index_base=start)
        x = host[r["best_idx"] - start] if r["best_idx"] >= 0 else np.zeros(C3_D)
        v, i, _, _ = comm.argmax(r["best_val"], r["best_idx"], x)
        return v, i, r["kernel_ms"], r["kernel"]

    # ---------------------------------------------------------------- C5: sharded NLML grid
    def c5_setup():
        X, Y = synth(5, C5_N, C5_D)
        allth = np.exp(np.random.RandomState(105).uniform(np.log(.1), np.log(3), size=(512, C5_D)))
        T = C5_T * world
        return X, Y, allth[:T] if T <= 512 else np.tile(allth, (T // 512 + 1, 1))[:T]

    def c5_step(X, Y, thetas):
        if comm is None:
            return nlml_grid(GaussianKernel_ard, thetas, X, Y, noise=1e-3, device=local_rank)
        return sharded_nlml_grid(GaussianKernel_ard, thetas, X, Y, comm, noise=1e-3, device=local_rank)

    out = None
    if args.config == "c3":
        GP, cand, host, start = c3_setup(C3_M_TOTAL)
        elapsed, outs = timed(lambda: c3_step(GP, cand, host, start), args.steps, args.warmup)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"best_value": outs[-1][0], "best_index": outs[-1][1]})
            kmean = float(np.mean([o[2] for o in outs])) * 1e-3
            out = dict(base)
            out.update({
                "metric": "EI evals/sec (N=2048 obs, D=8, Matern-5/2, 2^22 candidates sharded over the GPUs)",
                "value": float(C3_M_TOTAL) * args.steps / elapsed, "unit": "EI evals/s",
                "ms_per_step": elapsed / args.steps * 1e3, "scaling": "strong",
                "config": {"workload": "C3: N=2048 obs, D=8, MaternKernel5([.5, 1]), noise 0.1, EI xi=0.01 (libm erf), "
                                       "2^22 candidates in %d contiguous shard(s) resident in HBM, arg-max exchange each step" % world,
                           "n_obs": C3_N, "dim": C3_D, "candidates_total": C3_M_TOTAL,
                           "parallelism": "candidate-sharded x%d, replicated GP, 1 RCCL arg-max exchange/step" % world},
                "best": {"value": outs[-1][0], "index": int(outs[-1][1])},
                "roofline": attach_pmc(roofline_mfma(f_eval(C3_N, C3_D) * float(len(host)), kmean, kernel=outs[-1][3],
                                                     kernel_ms=kmean * 1e3, flops_per_eval=f_eval(C3_N, C3_D),
                                                     evals_per_launch=len(host), algorithmic_bytes_per_launch=(8 * C3_D + 16) * len(host)),
                                       "c3", float(len(host))),
            })
    elif args.config == "c5":
        X, Y, thetas = c5_setup()
        elapsed, outs = timed(lambda: c5_step(X, Y, thetas), args.steps, args.warmup)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"nlml_values": outs[-1][0], "nlml_argmin": outs[-1][1]})
            per_theta = elapsed / args.steps / C5_T            # each GPU does C5_T points per step
            out = dict(base)
            out.update({
                "metric": "NLML grid theta-points/sec (N=4096 obs, D=16, SE-ARD, 64 theta-points per GPU)",
                "value": float(C5_T * world) * args.steps / elapsed, "unit": "theta-points/s",
                "ms_per_step": elapsed / args.steps * 1e3, "scaling": "weak",
                "config": {"workload": "C5: N=4096 obs, D=16, GaussianKernel_ard theta-grid, noise 1e-3, 64 theta-points per GPU "
                                       "per step (host X,Y in, NLML values + argmin out), gathered by one all-reduce",
                           "n_obs": C5_N, "dim": C5_D, "theta_points_per_gpu": C5_T,
                           "parallelism": "theta-sharded x%d, 1 RCCL all-reduce/step" % world},
                "best": {"value": float(np.nanmin(outs[-1][0])), "index": int(outs[-1][1])},
                "roofline": attach_pmc(roofline_mfma(f_nlml(C5_N, C5_D), per_theta, kernel="chol_update3_kernel (dominant)",
                                                     ms_per_theta=per_theta * 1e3, flops_per_theta=f_nlml(C5_N, C5_D),
                                                     algorithmic_bytes_per_theta=24 * C5_N * C5_N,
                                                     note="whole grid step incl. K assembly, factorisation chain, reductions and the "
                                                          "gather; per-kernel times are in profiles/"), "c5"),
            })
    else:
        X, Y = synth(2, N_OBS, DIM)
        GP = GaussianProcess(GaussianKernel_ard([.3] * DIM), X, Y, noise=.1, device=local_rank)
        fit_ms = []
        for _ in range(5 if args.full else 0):              # GP-fit ms: host X,Y -> K, L, L^-1, alpha on device
            t0 = time.perf_counter()
            GP._fit_device()
            fit_ms.append((time.perf_counter() - t0) * 1e3)
        fit_dev_ms = GP.last_fit_ms()

        cand_host = np.random.RandomState(102 + rank).rand(M_PER_GPU, DIM)
        cand = DeviceArray.from_host(cand_host, local_rank)
        start = rank * M_PER_GPU

        def step():
            if getattr(comm, "device_exchange", False):   # RCCL: the local arg-max goes into the all-reduce without visiting the host
                r = sweep(GP, cand, acq='ei', xi=.01, native=True, index_base=start, exchange=comm)
                return r["global_val"], r["global_idx"], r["kernel_ms"], r["kernel"]
            r = sweep(GP, cand, acq='ei', xi=.01, native=True, index_base=start)
            if comm is not None:
                x = cand_host[r["best_idx"] - start] if r["best_idx"] >= 0 else np.zeros(DIM)
                v, i, _, _ = comm.argmax(r["best_val"], r["best_idx"], x)
                return v, i, r["kernel_ms"], r["kernel"]
            return r["best_val"], r["best_idx"], r["kernel_ms"], r["kernel"]

        elapsed, outs = timed(step, args.steps, args.warmup)
        if rank == 0:
            dump_outputs(args.dump_outputs, {"best_value": outs[-1][0], "best_index": outs[-1][1]})
            total = float(M_PER_GPU) * world * args.steps
            fe = f_eval(N_OBS, DIM)
            kmean = float(np.mean([o[2] for o in outs])) * 1e-3
            out = dict(base)
            out.update({
                "metric": "EI evals/sec (N=1024 obs, D=4, SE-ARD, 2^20 candidates/GPU sweep)",
                "value": total / elapsed, "unit": "EI evals/s", "ms_per_step": elapsed / args.steps * 1e3,
                "scaling": "weak",
                "config": {"workload": "C2: N=1024 obs, D=4, GaussianKernel_ard(0.3), noise 0.1, EI xi=0.01 (libm erf), "
                                       "2^20 candidates per GPU resident in HBM, arg-max to host each step",
                           "n_obs": N_OBS, "dim": DIM, "candidates_per_gpu": M_PER_GPU,
                           "parallelism": "candidate-sharded x%d, replicated GP, 1 RCCL arg-max exchange/step" % world},
                "best": {"value": outs[-1][0], "index": int(outs[-1][1])},
                "roofline": roofline_mfma(fe * float(M_PER_GPU), kmean, kernel=outs[-1][3], kernel_ms=kmean * 1e3,
                                          flops_per_eval=fe, evals_per_launch=M_PER_GPU),
            })
            if args.full:
                out["gp_fit_ms"] = {"host_to_ready_median": float(np.median(fit_ms)), "device_events": fit_dev_ms,
                                    "N": N_OBS, "D": DIM}
            j, src, sha = pmc_numbers()
            out["roofline"]["algorithmic_bytes_per_launch"] = (8 * DIM + 16) * M_PER_GPU
            out["roofline"]["kernel_source_sha"] = sha
            if j is not None:
                out["roofline"]["traffic"] = j.get("hbm_bytes_per_launch")
                out["roofline"]["traffic_source"] = "%s (rocprofv3 --pmc FETCH_SIZE x2, WRITE_SIZE; same kernel sources)" % src
                out["roofline"]["mfma_util_pct_pmc"] = j.get("mfma_util_pct")
            else:
                out["roofline"]["traffic_source"] = "no committed PMC summary matches this build of the kernel"

        if args.full and not args.no_extras:
            # ------------------------------------------------ the rest of the metric, on the same clock
            cfgs = {}
            # GP-fit ms (rank 0 is enough: the fit is single-GPU and replicated)
            if rank == 0:
                fits = {}
                for (n, d, kern) in ((1024, 4, GaussianKernel_ard([.3] * 4)), (2048, 8, MaternKernel5([.5, 1.0])),
                                     (4096, 16, GaussianKernel_ard([.3] * 16))):
                    Xf, Yf = synth(7, n, d)
                    g = GaussianProcess(kern, Xf, Yf, noise=.1, device=local_rank)
                    dev, host_ms = [], []
                    for _ in range(5):
                        t0 = time.perf_counter()
                        g._fit_device()
                        host_ms.append((time.perf_counter() - t0) * 1e3)
                        dev.append(g.last_fit_ms())
                    ms = float(np.median(dev))
                    fits["N%d_D%d" % (n, d)] = {"device_ms": ms, "host_to_ready_ms": float(np.median(host_ms)),
                                                "roofline": attach_pmc(roofline_mfma(f_fit(n, d), ms * 1e-3, flops_per_fit=f_fit(n, d),
                                                                                     algorithmic_bytes_per_fit=8 * n * d + 24 * n * n,
                                                                                     kernels="cov_fit + chol_pipe8 (pipelined block columns, two steps per pass over the trailing tiles, W riding along; from 4096 rows in super-panels of 16 block columns with chol_pack3 + chol_update3 deep updates of the columns beyond; two-level order + trinv_* from 6656 rows) + transpose_pack + gemv"),
                                                                       "fit%d" % n)}
                    del g
                    # one more observation through addData: an in-place extension of L, W and the packed copies
                    # (ibo_gp_extend) while the row padding has room -- reserve_rows keeps some -- else a refit
                    g = GaussianProcess(kern, Xf, Yf, noise=.1, device=local_rank, reserve_rows=8)
                    xa = np.random.RandomState(8).rand(3, d)
                    ext = []
                    for q in range(3):
                        t0 = time.perf_counter()
                        g.addData(xa[q], 0.0)
                        ext.append((time.perf_counter() - t0) * 1e3)
                    fits["N%d_D%d" % (n, d)]["addData_1_point_ms"] = float(np.median(ext))
                    del g
                cfgs["gp_fit"] = fits
            # C3: this rank's 2^19-candidate shard (at 8 GPUs this IS BASELINE configs[2])
            GP3, cand3, host3, start3 = c3_setup(C3_SHARD * world)
            el3, o3 = timed(lambda: c3_step(GP3, cand3, host3, start3), 5, 1)
            gms_all = []
            for _ in range(2):                                  # the first call also creates the hallucinated model's handle and
                barrier()                                       # the kept per-candidate state (12 MB): reported separately
                t0 = time.perf_counter()
                if comm is None:
                    gal = fastUCBGallery(GP3, [[0., 1.]] * C3_D, 8, candidates=cand3)
                else:
                    gal = sharded_gallery(GP3, [[0., 1.]] * C3_D, 8, cand3, start3, comm)
                gms_all.append(max_over_ranks((time.perf_counter() - t0) * 1e3))
            # "ms": the warm (second) call on the same model, "first_call_ms": the first one -- BENCH_r03's keys and meaning (BENCH_r04 had
            # them swapped under "ms" / "warm_ms": compare that round through "first_call_ms")
            gms_first, gms = gms_all[0], gms_all[1]
            if rank == 0:
                k3 = float(np.mean([o[2] for o in o3])) * 1e-3
                gal = np.array(gal)
                cfgs["c3_shard_sweep"] = {
                    "workload": "N=2048, D=8, Matern-5/2, EI over 2^19 candidates per GPU (x%d), 5 steps" % world,
                    "value": float(C3_SHARD * world) * 5 / el3, "unit": "EI evals/s", "ms_per_step": el3 / 5 * 1e3,
                    "gp_fit_device_ms": GP3.last_fit_ms(),
                    "roofline": attach_pmc(roofline_mfma(f_eval(C3_N, C3_D) * float(C3_SHARD), k3, kernel=o3[-1][3],
                                                         kernel_ms=k3 * 1e3, flops_per_eval=f_eval(C3_N, C3_D),
                                                         evals_per_launch=C3_SHARD, algorithmic_bytes_per_launch=(8 * C3_D + 16) * C3_SHARD),
                                           "c3", float(C3_SHARD))}
                cfgs["c3_gallery8"] = {"workload": "fastUCBGallery(N=8) on the same GP and shard(s): 7 rounds of DIRECT + "
                                                   "sharded sweep + exchange + hallucinated addData",
                                       "ms": gms, "first_call_ms": gms_first, "ms_key_means": "second call on the same model (as in round 3; round 4 stored the first call here)",
                                       "min_pairwise_distance": float(min(
                                           np.linalg.norm(gal[i] - gal[j]) for i in range(8) for j in range(i)))}
            del GP3, cand3
            # C5: 64 theta-points per GPU
            X5, Y5, th5 = c5_setup()
            el5, o5 = timed(lambda: c5_step(X5, Y5, th5), 2, 1)   # the warm-up step sizes the batch workspace
            if rank == 0:
                per = el5 / 2 / C5_T
                cfgs["c5_nlml_grid"] = {
                    "workload": "N=4096, D=16, SE-ARD, 64 theta-points per GPU (x%d), host X,Y in, values + argmin out" % world,
                    "ms_total": el5 / 2 * 1e3, "ms_per_theta": per * 1e3, "argmin": int(o5[-1][1]),
                    "n_not_pd": int(np.sum(~np.isfinite(o5[-1][0]))),
                    "roofline": attach_pmc(roofline_mfma(f_nlml(C5_N, C5_D), per, flops_per_theta=f_nlml(C5_N, C5_D),
                                                         algorithmic_bytes_per_theta=24 * C5_N * C5_N,
                                                         kernels="cov_grid_mfma (exponent on the MFMA unit) + left-looking chol_update3 (dominant) + chol_panel_fused + tail + reduce"),
                                           "c5")}
            _lib.trim(local_rank)
            # hyper-parameter learning's inner loop (ego/gaussianprocess/trainhyper.py:77-95,130-136): one NLML value + gradient
            # w.r.t. every log length scale = fit chain with W riding along, K^-1 = W^T W, the contraction with dK/dtheta.  Host X, Y in,
            # value + gradient out; rank 0 (single-GPU, replicated)
            if rank == 0:
                from ibo_amd.gaussianprocess.trainhyper import marginalLikelihood
                ng = {}
                for n, d in ((1024, 16), (4096, 16)):
                    Xg, Yg = synth(9, n, d)
                    kern = GaussianKernel_ard([.5] * d)
                    ms = []
                    for _ in range(6):
                        t0 = time.perf_counter()
                        marginalLikelihood(kern, Xg, Yg, d, True, noise=1e-3)
                        ms.append((time.perf_counter() - t0) * 1e3)
                    per = float(np.median(ms[1:]))
                    fl = f_nlml(n, d) + 2.0 * n ** 3 / 3.0 + d * 2.0 * n * n          # with gradient add 2N^3/3 + D 2N^2
                    ng["N%d_D%d" % (n, d)] = {"ms": per, "first_call_ms": ms[0],
                                              "roofline": attach_pmc(roofline_mfma(fl, per * 1e-3, flops_per_evaluation=fl,
                                                                                   algorithmic_bytes_per_evaluation=8 * n * d + 4 * 8 * n * n,
                                                                                   kernels="cov_fit + chol_pipe8 (W riding along; super-panels + chol_update3 from 4096 rows) + transpose_pack + K^-1 = W^T W (wtw_kernel; from 1792 rows syrk3_pack + chol_update3 in pieces + syrk3_sum) + nlml_grad_fast + reductions"),
                                                                     "learn%d" % n)}
                cfgs["nlml_grad"] = {"workload": "one marginalLikelihood(..., computeGradient=True) evaluation, SE-ARD, D = 16 length scales, host X, Y in, value + gradient out (wall, median of 5)",
                                     "results": ng}
                _lib.trim(local_rank)
            # C4: preference GP, one GPU only (the MAP is a sequential Newton iteration)
            if world == 1:
                rs = np.random.RandomState(4)
                pts = rs.rand(1024, 6)
                prefs = []
                for i in range(512):
                    a_, b_ = pts[2 * i], pts[2 * i + 1]
                    prefs.append((a_, b_, 0) if hartman6(a_) > hartman6(b_) else (b_, a_, 0))
                pref_ms = []
                for _ in range(3):                  # the first call pays for this handle type's buffers and code objects
                    t0 = time.perf_counter()
                    PG = PrefGaussianProcess(GaussianKernel_ard([0.53, 0.57, 2.5, 0.34, 0.27, 0.35]), prefs, device=local_rank)
                    pref_ms.append((time.perf_counter() - t0) * 1e3)
                pms = min(pref_ms[1:])
                cand4 = DeviceArray.from_host(np.random.RandomState(104).rand(1 << 20, 6), local_rank)
                g4 = []
                for _ in range(2):
                    t0 = time.perf_counter()
                    fastUCBGallery(PG, [[0., 1.]] * 6, 8, candidates=cand4)
                    g4.append((time.perf_counter() - t0) * 1e3)
                cfgs["c4_prefgp"] = {"workload": "PrefGaussianProcess, 512 pairs -> 1024 points, D=6; gallery of 8 over 2^20 candidates",
                                     "addPreferences_ms": pms, "addPreferences_first_call_ms": pref_ms[0],
                                     "gallery8_ms": g4[1], "gallery8_first_call_ms": g4[0]}
                del PG, cand4
                # The drop-in symbol acqmaxGP (include/ibo_abi.h section A) as the reference's cdirectGP calls it
                # (ego/acquisition/__init__.py:385-436: inv(R) formed by the caller, default budget 50 iterations / 10 000 samples), at
                # C2's and C3's model sizes, both routes: "exact" = libego's operation order (csrc/legacy.hip, the default: the
                # reference's numbers bit for bit), "fast" = inv(R) factored on the device + the MFMA sweep kernels (within 1e-6 of
                # libego on well-conditioned data only).  Whole-call wall time, host buffers in (the 8 N^2-byte inv(R) upload included).
                import ctypes as _ct0
                libc = _ct0.CDLL(None); libc.free.argtypes = [_ct0.c_void_p]

                def legacy_ms(Xl, Yl, kern, ktype, hyper, what):
                    g = GaussianProcess(kern, Xl, Yl, noise=.1, device=local_rank)
                    invR = _lib.f64(np.linalg.inv(np.array(g.R)))
                    d = Xl.shape[1]
                    lb, ub, Xc, Yc, hy, one = _lib.f64([0.] * d), _lib.f64([1.] * d), _lib.f64(Xl), _lib.f64(Yl), _lib.f64(hyper), _lib.f64([0.])
                    res = {"workload": what}
                    for route, key in ((1, "exact"), (0, "fast")):
                        _lib.check(_lib.lib.ibo_set_option(b"legacy_exact", route))
                        ms = []
                        try:
                            for _ in range(4):
                                t0 = time.perf_counter()
                                r = _lib.lib.acqmaxGP(d, _lib.dp(lb), _lib.dp(ub), _lib.dp(invR), _lib.dp(Xc), _lib.dp(Yc), len(Yc), 0, ktype, _lib.dp(hy),
                                                      0, _lib.dp(one), _lib.dp(one), 0., _lib.dp(one), _lib.dp(one), .01, .1, 50, 30, 10000)
                                ms.append((time.perf_counter() - t0) * 1e3)
                                if not bool(r):
                                    raise RuntimeError("acqmaxGP returned NULL")
                                res[key + "_EI"] = -r[0]
                                libc.free(r)
                        finally:
                            _lib.check(_lib.lib.ibo_set_option(b"legacy_exact", 1))
                        res[key + "_ms"] = float(np.median(ms[1:]))
                    res["rel_diff_fast_vs_exact"] = float(abs(res["fast_EI"] - res["exact_EI"]) / max(abs(res["exact_EI"]), 1e-300))
                    res["default_route"] = "exact"
                    return res
                Xl, Yl = synth(2, N_OBS, DIM)
                cfgs["legacy_acqmaxGP_c2"] = legacy_ms(Xl, Yl, GaussianKernel_ard([.3] * DIM), 0, [.3] * DIM,
                                                       "acqmaxGP, EI xi=.01, N=1024, D=4, SE-ARD, noise .1, maxiter 50 / maxsample 10000, inv(R) from the host")
                Xl, Yl = synth(3, C3_N, C3_D)
                cfgs["legacy_acqmaxGP_c3"] = legacy_ms(Xl, Yl, MaternKernel5([.5, 1.0]), 3, [.5, 1.0],
                                                       "acqmaxGP, EI xi=.01, N=2048, D=8, Matern-5/2, noise .1, maxiter 50 / maxsample 10000, inv(R) from the host")
                # the sweep kernel against the input dimension (N = 1024, 2^18 candidates: a quarter of the headline batch, so the
                # tail of the tile rounds weighs more): D = 17..32 take a 32-coordinate row layout and 6..9 k4-steps of the exponent GEMM
                from ibo_amd.acquisition import sweep as _sweep
                dims = {}
                for d in (8, 16, 24, 32):
                    Xd, Yd = synth(11, 1024, d)
                    cd = DeviceArray.from_host(np.random.RandomState(111).rand(1 << 18, d), local_rank)
                    for name, kern in (("se_ard", GaussianKernel_ard([.3 * np.sqrt(d / 4.)] * d)), ("matern52", MaternKernel5([.5 * np.sqrt(d / 4.), 1.0]))):
                        g = GaussianProcess(kern, Xd, Yd, noise=.1, device=local_rank)
                        for _ in range(2):
                            _sweep(g, cd)
                        ms = float(np.mean([_sweep(g, cd)["kernel_ms"] for _ in range(5)]))
                        dims["D%d_%s" % (d, name)] = {"kernel_ms": ms, "frac": f_eval(1024, d) * float(1 << 18) / (ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
                        del g
                    del cd
                cfgs["sweep_by_dimension"] = {"workload": "N=1024, EI over 2^18 candidates, kernel time (HIP events)", "results": dims}
                # The exact arg-max WITHOUT the per-candidate values (round-2 review, item 9) -- under its own key, never the headline:
                # work is skipped.  ibo_acq_sweep_incremental on a fresh array forms its state over the first half of W's rows and runs
                # the second half only for the 32-candidate tiles whose EI bound reaches the best complete value (what the gallery's
                # first round does); the winner is the full sweep's.
                import ctypes as _ct

                def argmax_only(GPm, cand_np, full_ms, full_best, what, **kw):
                    am = []
                    for _ in range(4):
                        ca = DeviceArray.from_host(cand_np, local_rank)        # a new array: no kept state
                        _lib.check(_lib.lib.ibo_device_synchronize(local_rank))
                        t0 = time.perf_counter()
                        ra = sweep(GPm, ca, incremental=True, **kw)
                        am.append((time.perf_counter() - t0) * 1e3)
                        nl = _ct.c_int(); sp = (_ct.c_int * 3)(); cnt = (_ct.c_int64 * 4)()
                        _lib.check(_lib.lib.ibo_sweep_state_levels(GPm._handle(), _ct.byref(nl), sp, cnt))
                        del ca
                    ms = float(np.median(am[1:]))
                    tiles = int(sum(list(cnt)[:nl.value]))
                    return {"workload": what, "ms": ms, "candidates_per_s": len(cand_np) / ms * 1e3, "full_sweep_ms": full_ms,
                            "levels": int(nl.value), "level_starts_at_row": [0] + list(sp)[:nl.value - 1],
                            "tiles": tiles, "tiles_standing_at_each_level": list(cnt)[:nl.value],
                            "tiles_complete": int(cnt[nl.value - 1]), "last_level_skipped_frac": 1.0 - cnt[nl.value - 1] / max(1, tiles),
                            "same_index_as_full_sweep": bool(ra["best_idx"] == full_best[1]),
                            "value_rel_diff_to_full_sweep": float(abs(ra["best_val"] - full_best[0]) / abs(full_best[0]))}
                cfgs["argmax_only"] = argmax_only(GP, cand_host, elapsed / args.steps * 1e3, outs[-1],
                                                  "C2 shape, arg-max of EI only: kept-state sweep in levels of W's rows (first call on a new array)",
                                                  acq='ei', xi=.01, native=True, index_base=start)
                # the north-star shape (N = 2048, D = 8, Matern-5/2) on one GPU: 2^19 candidates
                GPn, candn, hostn, startn = c3_setup(C3_SHARD)
                fulln = sweep(GPn, candn, acq='ei', xi=.3, native=True)
                cfgs["argmax_only_c3"] = argmax_only(GPn, hostn, float(fulln["kernel_ms"]), (fulln["best_val"], fulln["best_idx"]),
                                                     "N=2048, D=8, Matern-5/2, arg-max of EI only over 2^19 candidates (first call on a new array)",
                                                     acq='ei', xi=.3, native=True)
                del GPn, candn
            if rank == 0:
                out["configs"] = cfgs
        if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(X, Y, cand_host)

    if rank == 0:
        # what an outside observer's busy-GPU samples can be held against: device time measured with HIP events over the whole
        # run (fits, sweeps, grids, gradients; DIRECT's small batches and copies are not event-timed), beside the run's wall time
        out["gpu_kernel_s_total"] = _lib.gpu_time_ms(local_rank) * 1e-3
        out["wall_s_total"] = time.perf_counter() - T_START
        os.write(json_fd, (json.dumps(out) + "\n").encode())
    if comm is not None:
        comm.barrier()
        comm.close()
        if rank == 0 and id_path and not os.environ.get("IBO_BENCH_CHILD"):
            try:
                os.unlink(id_path)
            except OSError:
                pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--config", choices=("c2", "c3", "c5"), default="c2")
    ap.add_argument("--full", action="store_true",
                    help="also measure GP-fit ms, the `configs` object and the CPU baseline (default config only)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step returned as DIR/<name>.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the `configs` object (fit / C3 / C4 / C5 numbers)")
    args = ap.parse_args()
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")
    launched = "WORLD_SIZE" in os.environ or "RANK" in os.environ
    if not launched and (args.gpus > 1 or os.environ.get("IBO_BENCH_FORCE_SPAWN")):
        # no GPU call has been made in this process (ibo_amd is imported by the workers only)
        sys.exit(self_launch(args.gpus, sys.argv[1:]))
    worker(args)


if __name__ == "__main__":
    main()
