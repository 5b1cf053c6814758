"""OFF-forward benchmark (BASELINE.json metric: OFF-forward clips/sec, 7-seg 224x224).

    python bench.py                                   # 1 GPU, BASELINE config 2
    python bench.py --gpus N --steps K --warmup W     # starts its own N ranks (one per GPU, RCCL)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W          # what the driver runs
    python bench.py --gpus 2 --oversubscribe          # 2 ranks on ONE GPU: exercises the N > 1 code path on a 1-GPU
                                                      # box (scores exchanged over gloo, host-staged: RCCL refuses two
                                                      # ranks per device) -- NOT a scaling number

A "step" is one pass of the OFF sub-network forward (liboffk: nine OFF units, fusion @28/@14/@7,
three heads) over one batch of synthetic BN-Inception feature maps already resident in HBM.
N = 1 is BASELINE config 2 (RGB_OFF, B = 64 clips x 7 segments).  N > 1 is config 4: every rank
owns 64 clips (weak scaling, no data-path collective), takes the SegmentConsensus average per
clip and the per-clip scores are exchanged once per step with one RCCL all-gather over xGMI.
Rank 0 prints ONE JSON line.

    python bench.py --collective-smoke                # N = 1 with a single-rank RCCL group: librccl init + the per-step score
                                                      # exchange (all-gather AND the all-reduce form) inside the timed step --
                                                      # NOT a scaling number (a dev box has one GPU)

What the line's `value` is (round 6, VERDICT r05's ruling): the library's split-fp32 mode (OFFK_PRECISION_F32SPLIT: every fp32 operand
as three bf16 planes = the fp32 value exactly, six exact plane products on the bf16 matrix pipe, fp32 accumulation -- the units kernel, the
batched GEMMs of every conv on a Winograd path, the 1x1 convs on 7x7 maps; measured error against fp64 below the fp32 pipe's on every
input kind, asserted in tests/test_gpu_split.py) at the full --steps.  With --full the fp32-MFMA-pipe mode of the same library (v_mfma_f32_*)
is timed beside it as `fp32_pipe_mode`.  `--precision fp32` swaps the two.

A plain run times the headline forward only: set-up, --warmup untimed steps, --steps timed steps, the line.  Everything else it
can measure or check runs with --full: the profiled second loop (stage times, the standalone K2 launches of the roofline object,
the per-launch roofline_in_path), the other arithmetic mode, both modes' error tables against fp64, the Flow and two-stream
configs, units_training, the single-rank RCCL smoke object, the CPU baseline and, with a score exchange on the step, the check
of the exchanged scores (exchange_ok, --dump-scores).

    python bench.py --full                            # every object above in the line and in bench_detail.json
    python bench.py --dump-outputs DIR                # + DIR/logits_{7,14,28}.npy: the timed path's outputs of its last step

Output: the ONE stdout line is a compact object (< 8 KB, `compact_line`, pinned by tests/test_bench_line.py); everything else
(per-launch tables, stage times, both modes' error tables, the CPU baseline's operating points, units_training) goes to
bench_detail.json next to this script and to stderr.
"""
import argparse
import contextlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--batch", type=int, default=64, help="clips per GPU")
    ap.add_argument("--length", type=int, default=7)
    ap.add_argument("--variant", choices=("rgb", "flow"), default="rgb")
    ap.add_argument("--precision", choices=("fp32", "f32split"), default="f32split",
                    help="arithmetic of the headline value (f32split = fp32 operands as three bf16 planes on the bf16 pipe, ruled "
                         "fp32-equivalent in VERDICT r05; fp32 = the fp32 MFMA pipe); with --full the other mode is reported beside it at "
                         "N = 1 with both modes' measured error against fp64")
    ap.add_argument("--detail", default=os.path.join(ROOT, "bench_detail.json"), metavar="PATH",
                    help="where rank 0 writes the full result object (the stdout line is its compact form)")
    ap.add_argument("--cpu-clips", type=int, default=64, help="clips in the large CPU-baseline sample (0 = skip the CPU baseline)")
    ap.add_argument("--no-secondary", action="store_true", help="--full at N = 1: skip the f32split / training / CPU-baseline objects")
    ap.add_argument("--collective", choices=("allgather", "allreduce"), default="allgather",
                    help="N > 1: the one exchange of per-clip scores (allreduce = zeroed [B,101] buffer + sum, north_star's wording)")
    ap.add_argument("--collective-smoke", action="store_true",
                    help="N = 1: create a single-rank RCCL process group in this process and run the per-step score exchange "
                         "(dist.py: all-gather and the all-reduce form) inside the timed step.  Executes librccl on the one GPU "
                         "there is; labelled as a smoke run, not a scaling number")
    ap.add_argument("--oversubscribe", action="store_true",
                    help="N > 1 on a box with fewer GPUs than ranks: ranks share devices (rank %% device_count), scores go "
                         "over a gloo group (host-staged).  Exercises the multi-rank code path; not a scaling measurement")
    ap.add_argument("--dump-scores", default=None, metavar="PATH",
                    help="with a score exchange on the step (N > 1 or --collective-smoke): rank 0 writes the exchanged scores of the "
                         "verification step, [3 heads (7, 14, 28)][world * clips][classes], to PATH (.npy) -- "
                         "tests/test_gpu_two_ranks.py compares them with the oracle called per shard (needs --full)")
    ap.add_argument("--full", action="store_true",
                    help="besides the headline timing: the profiled loop, the roofline objects, the secondary measurements, the CPU "
                         "baseline and the check of the score exchange (see the module docstring)")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, rank 0 writes what the last timed step computed to DIR/logits_{7,14,28}.npy (float32): "
                         "the three heads' scores [rows][classes], with a score exchange on the step the exchanged scores of every rank "
                         "[world * clips][classes]")
    args = ap.parse_args()
    if args.dump_scores and not args.full:
        ap.error("--dump-scores is written by the check of the score exchange, which runs with --full")
    return args


def launch_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a torch.distributed.run CHILD process.
    Nothing in this process has touched the GPU (torch is not even imported yet), and the child is spawned, never
    exec'ed over this process.  Exit code = the child's."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    return subprocess.run(cmd, env=env).returncode


ARGS = parse_args() if __name__ == "__main__" else None
if ARGS is not None and "RANK" not in os.environ and ARGS.gpus > 1:
    sys.exit(launch_ranks(ARGS))

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import hashlib  # noqa: E402
import numpy as np  # noqa: E402
import statistics  # noqa: E402
import time  # noqa: E402

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

import offk_amd  # noqa: E402,F401
from offk_amd import dist as odist, runtime, spec, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec); ~6.3 TB/s achievable
K2_PER_PAIR = 4           # standalone K2 launches per HIP-event pair (roofline object)
MFMA_F32_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md: fp32-input MFMA peak
BF16_DENSE_PEAK_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense bf16 MFMA peak (measured on these operands: ~2.1 PF, profiles/r05/probe_split_mfma.txt)
DTYPES = {"fp32": "f32",
          "f32split": "f32 (split-fp32: every fp32 operand as three bf16 planes = the fp32 value exactly, six exact plane products "
                      "on the bf16 MFMA pipe, f32 accumulate)"}


def cpu_baseline(feats_np, weights, length, variant, clips_large):
    """The oracle (a port of the reference's op sequence, bit-exact against it in the dev container) timed on this
    box's host cores -- reported beside the GPU number only.  SURVEY.md 8(d): at B = 1 and at the bench batch.
    torch's intra-op threading does not scale to every logical CPU on these small convs, so a few thread counts are
    tried at each size (one warm-up + one run each) and the fastest is used: the baseline is the best the host
    does, not a strawman."""
    from oracle import off_oracle as orc
    w = orc.to_torch_weights(weights)

    def run(clips):
        x = [torch.from_numpy(f[:clips * length]) for f in feats_np]
        t0 = time.perf_counter()
        orc.off_forward(x, w, clips, length, variant, orc.SLICE_FLAT)
        return time.perf_counter() - t0

    ncpu = usable_cpus()

    def best_threads(clips, cands):
        best_t, best_n, sweep = None, None, {}
        for n in cands:
            if n > ncpu:
                continue
            torch.set_num_threads(n)
            run(clips)
            t = run(clips)
            sweep[n] = clips / t
            if best_t is None or t < best_t:
                best_t, best_n = t, n
        return best_n, sweep

    with torch.no_grad():
        n1, sweep1 = best_threads(1, sorted({min(4, ncpu), min(8, ncpu), 16, 32}))
        torch.set_num_threads(n1)
        t1 = statistics.median([run(1) for _ in range(5)])
        best_n, sweep = best_threads(clips_large, sorted({min(16, ncpu), 32, 64, max(1, ncpu // 2)}))
        torch.set_num_threads(best_n)
        tl = statistics.median([run(clips_large) for _ in range(3)])
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        pass
    large = {"value": clips_large / tl, "unit": "clips/s", "cores": best_n, "sec_per_forward": tl,
             "sample": "first %d clips x %d segments in one call, 1 warm-up, median of 3 at the fastest thread count"
                       % (clips_large, length), "clips_per_s_by_threads": sweep}
    one = {"value": 1.0 / t1, "unit": "clips/s", "cores": n1, "sec_per_forward": t1,
           "sample": "1 clip x %d segments per call, median of 5 at the fastest thread count" % length,
           "clips_per_s_by_threads": sweep1}
    conc = cpu_concurrent(length, variant)
    best = max((one, large, conc), key=lambda r: r["value"])     # `value` = the host's BEST operating point, not the bench batch
    return {"value": best["value"], "unit": "clips/s", "cores": best["cores"], "kind": "port",
            "sample": "oracle/off_oracle.py (torch CPU ops, bit-exact vs the reference import) on the same synthetic maps; "
                      "the fastest of three operating points: " + best["sample"],
            "batch_1": one, "batch_large": large, "concurrent_batch_1": conc, "cpu_model": model,
            "host_logical_cpus": os.cpu_count(), "usable_cpus": usable_cpus()}


_CPU_WORKER = r"""
import sys, time
sys.path.insert(0, %(root)r)
import torch
torch.set_num_threads(%(threads)d)
import offk_amd  # noqa: F401
from offk_amd import spec, synth
from oracle import off_oracle as orc
L, variant = %(length)d, %(variant)d
w = orc.to_torch_weights(synth.make_weights(variant))
x = [torch.from_numpy(f) for f in synth.make_features(1, L, 2)]
with torch.no_grad():
    for _ in range(2):
        orc.off_forward(x, w, 1, L, variant, orc.SLICE_FLAT)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < %(seconds)f:
        orc.off_forward(x, w, 1, L, variant, orc.SLICE_FLAT)
        n += 1
    print(n / (time.perf_counter() - t0))
"""


def usable_cpus():
    """CPUs this process may actually run on: the affinity mask, capped by the cgroup's cpu.max quota (a GPU box hands a
    job a share of the host, e.g. 16 of 256 logical CPUs)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def make_features(batch, length, config_id, clip_offset):
    """synth.make_features in chunks on a thread pool: one bench batch is 2 GB of maps, ~14 s on one core, and that is set-up
    time of every run.  The generator is counter-based (element i of a site is counter i of its stream), so a chunk is
    synth.feature_values of its own counter range and the maps are bit-identical to synth.make_features'."""
    from concurrent.futures import ThreadPoolExecutor
    chunk = 1 << 21
    feats, jobs = [], []
    for si, (_name, C, H) in enumerate(spec.SITES):
        per_clip = length * C * H * H
        v = np.empty(batch * per_clip, dtype=np.float32)
        for o in range(0, v.size, chunk):
            jobs.append((v, synth.feature_seed(config_id, si), clip_offset * per_clip + o, o, min(chunk, v.size - o)))
        feats.append(v.reshape(batch * length, C, H, H))

    def fill(job):
        v, seed, start, o, n = job
        v[o:o + n] = synth.feature_values(seed, start, n)

    with ThreadPoolExecutor(max_workers=min(16, usable_cpus())) as ex:
        list(ex.map(fill, jobs))
    return feats


def cpu_concurrent(length, variant, seconds=6.0):
    """The host's throughput operating point: N independent single-clip oracle processes side by side, N x threads = the CPUs
    this job may use (one process at a time leaves most of them idle on these small convs).  Tried at 2 and 4 threads per
    process; the faster split is reported."""
    ncpu = usable_cpus()
    best = None
    for threads in (2, 4):
        procs = max(1, ncpu // threads)
        src = _CPU_WORKER % {"root": ROOT, "threads": threads, "length": length, "variant": variant, "seconds": seconds}
        env = dict(os.environ, OMP_NUM_THREADS=str(threads), MKL_NUM_THREADS=str(threads), HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
        ps = [subprocess.Popen([sys.executable, "-c", src], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, env=env, text=True)
              for _ in range(procs)]
        rates = []
        for q in ps:
            o, _ = q.communicate()
            try:
                rates.append(float(o.strip().splitlines()[-1]))
            except (ValueError, IndexError):
                rates.append(0.0)
        rec = {"value": sum(rates), "unit": "clips/s", "processes": procs, "threads_per_process": threads, "cores": procs * threads,
               "sample": "%d concurrent processes x %d threads, each looping 1 clip x %d segments per call for %.0f s (2 warm-ups)"
                         % (procs, threads, length, seconds)}
        if best is None or rec["value"] > best["value"]:
            best = rec
    best["usable_cpus"] = ncpu
    return best


def measured_traffic(batch, length, variant):
    """HBM bytes per K2 launch from rocprofv3 PMC passes (FETCH_SIZE doubled per the gfx950 correction in
    MI355X_MICROARCH.md + WRITE_SIZE), as tools/measure_k2_traffic.py recorded them in profiles/k2_traffic.json.
    The record carries the sha256 of the kernel source it was collected on: for any other kernel text (or another
    configuration) the field is null -- a stale constant is not a measurement."""
    try:
        rec = json.load(open(os.path.join(ROOT, "profiles", "k2_traffic.json")))
        src = open(os.path.join(ROOT, "optical-flow-guided-feature-pytorch_amd", "csrc", "sobel_tdiff.hip"), "rb").read()
    except (OSError, ValueError):
        return None
    if rec.get("kernel_source_sha256") != hashlib.sha256(src).hexdigest():
        return None
    if rec.get("batch") == batch and rec.get("length") == length and rec.get("variant") == variant:
        return rec.get("hbm_bytes_per_launch")
    return None


def launch_work(P):
    """Algorithmic FLOPs per launch group of the per-launch trace (names: offk_api.hip trace_mark), P = B * (L - 1) pairs,
    2 * MACs as in BASELINE.md section 3.  Merged convs = main 1x1 + residual-branch 1x1 in one K-concatenated launch."""
    d = {}
    for key, co, ci, k, _s, _p in spec.FUSION_CONVS:
        hw = 196 if key.endswith(("_28", "_28a", "_28b", "_28c")) else 49
        d[key] = 2.0 * P * hw * co * ci * k * k
    d["merged_28a"] = d["motion_conv3_trans_28a"] + d["motion_conv_branch_28a"]
    d["merged_14a"] = d["motion_conv3_trans_14a"] + d["motion_conv_expand_trans_14a"]
    d["merged_7"] = d["motion_conv3_trans"] + d["motion_conv_branch_trans"]
    return d


WINOGRAD_CONVS = ("motion_conv2_trans_14a", "motion_conv2_trans_14b", "motion_conv3_trans_14b", "motion_conv_trans",
                  "motion_conv2_trans", "motion_conv_trans_14", "motion_conv_trans_28")
POLYPHASE_MIN_PAIRS = {"motion_conv_trans_14": 40, "motion_conv_trans_28": 12}   # the polyphase forms are used from this many pairs (offk_api.hip)


def winograd_gemm_flops(P, key):
    """FLOPs of the batched GEMMs [P images][K] x [K][Co] of a conv on the Winograd path: 121 points with K = Ci for a 3x3 /
    stride 1 conv on 7x7 maps, four K groups for the polyphase forms (four phase images concatenated along K)."""
    co, ci, k = next((c, i, kk) for k_, c, i, kk, _s, _p in spec.FUSION_CONVS if k_ == key)
    if k == 7:      # F(5x5, 4x4) on four 14x14 phase images: 9 tiles per 14x14 output map, 225 of 256 (point, phase) products
        return 2.0 * 9 * P * 225 * ci * co
    # a 7x7 map = four tiles, F(4, 3) x F(3, 3) per axis: 121 points per image; polyphase 5x5: 400 of the 484 (point, phase)
    # products -- the others have an identically zero transformed kernel and are skipped
    return 2.0 * P * (400 * ci if k == 5 else 121 * ci) * co


def winograd_saved_flops(P, precision="fp32"):
    """Direct-conv FLOPs minus the FLOPs of the batched GEMMs for the convs the forward runs in a Winograd form
    (csrc/winograd.hip, csrc/winograd7.hip; the 3x3 convs inside the bottleneck chains only in the fp32 kernel, chain_fused.hip --
    a split-fp32 handle runs them direct on the bf16 pipe, chain_split.hip)."""
    w = launch_work(P)
    on = [k for k in WINOGRAD_CONVS if not (k == "motion_conv_trans_28" and os.environ.get("OFFK_WINOGRAD_7X7", "1") == "0")
          and not (k == "motion_conv_trans_14" and os.environ.get("OFFK_WINOGRAD_5X5", "1") == "0")
          and not P < POLYPHASE_MIN_PAIRS.get(k, 0)]
    saved = sum(w[k] - winograd_gemm_flops(P, k) for k in on)
    return saved + sum(w[k] - chain_winograd_flops(P) for k in chain_winograd_convs(P, precision))


CHAIN_MIN_PAIRS = 72      # one launch per bottleneck chain of fusion@28 from this many pairs (offk_api.hip, OFFK_CHAIN)


def split_chains(P, precision):
    """A split-fp32 handle runs the bottleneck chains on chain_split.hip (offk_api.hip: OFFK_SPLIT_CHAIN, from the chain gate on)."""
    e = os.environ
    gate = int(e["OFFK_CHAIN"]) if e.get("OFFK_CHAIN", "").isdigit() and int(e["OFFK_CHAIN"]) > 1 else 1      # (split handles: from the first pair on)
    return (precision == "f32split" and e.get("OFFK_SPLIT_CHAIN", "1") != "0" and e.get("OFFK_CHAIN", "1") != "0" and
            e.get("OFFK_WINOGRAD", "1") != "0" and P >= gate)


def chain_winograd_convs(P, precision="fp32"):
    """The 3x3 convs that run in Winograd F(2x2, 3x3) form inside chain14_kernel (chain_fused.hip): the default from the chain gate on."""
    if split_chains(P, precision):
        return ()
    e = os.environ
    gate = int(e["OFFK_CHAIN"]) if e.get("OFFK_CHAIN", "").isdigit() and int(e["OFFK_CHAIN"]) > 1 else CHAIN_MIN_PAIRS
    if e.get("OFFK_CHAIN", "1") == "0" or e.get("OFFK_CHAIN_WINO", "1") == "0" or e.get("OFFK_WINOGRAD", "1") == "0" or P < gate:
        return ()
    return ("motion_conv2_trans_28a", "motion_conv2_trans_28b", "motion_conv2_trans_28c")


def chain_winograd_flops(P):
    """FLOPs of the sixteen point GEMMs of a 64 -> 64 3x3 conv on 14x14 maps in F(2x2, 3x3): 7 x 7 tiles per image, 1 / 2.25 of the direct
    conv's (the kernel multiplies 32 tile slots per half image for its 28 tiles; as everywhere, padding is not counted as work)."""
    return 2.0 * P * 49 * 16 * 64 * 64


SPLIT_FRAC_OF = "six bf16 products per fp32 product / 2.5 PF dense bf16"
SPLIT_1X1_LAUNCHES = ("merged_14a", "merged_7", "motion_conv1_trans_14b", "motion_conv_branch_28a")


def roofline_in_path(h, arr, out, B, L, precision, steps):
    """What bounds the kernels the DEFAULT forward launches: a third loop with the library's per-launch trace on (one HIP
    event in front of every launch group, heads folded back onto the main stream).  HBM-bound: the S-blocks of K2 (the only
    part of the roofline object that the fused inference path still runs); MFMA-bound: K1T and every fusion conv, each
    against the fp32-MFMA peak with its algorithmic FLOPs.  Events between short kernels add a few us each: the small-conv
    fractions are lower bounds, rocprofv3's kernel trace (profiles/) is the cross-check."""
    P = B * (L - 1)
    h.set_profiling(2)
    h.launch_times(reset=True)
    for _ in range(steps):
        h.forward_into(arr, out[0], out[1], out[2])
    torch.cuda.synchronize()
    lt = h.launch_times(reset=True)
    h.set_profiling(0)
    work = launch_work(P)
    unit_f, _fus = spec.flops_per_clip(L)
    hw = sum(H * H for _n, _c, H in spec.SITES)
    dw_f = 2.0 * P * hw * spec.DOWN_CH * 9
    peak = MFMA_F32_PEAK_TFLOPS          # (f32split: the launches on the bf16 pipe are priced against the bf16 peak, `frac_of` says so)
    kernels, small_ms, small_fl = [], 0.0, 0.0
    big = ("motion_conv_trans_28", "motion_conv_trans_14", "motion_conv_trans")
    for name, (ms, calls) in lt.items():
        avg = ms / max(calls, 1)
        rec = {"launch": name, "avg_ms": avg, "calls": calls}
        if name.startswith("units:pw_tdiff") or name.startswith("units:pw_reduce"):
            fl = unit_f * B - dw_f
            rec.update(bound="mfma", flops=fl, achieved_tflops=fl / avg / 1e9, frac=fl / avg / 1e9 / peak)
            if precision == "f32split" and name.startswith("units:pw_tdiff"):
                # split-fp32: six bf16 plane products per fp32 product; the bound that matters beside the pipe is HBM (X in, T / D out)
                nbytes = B * (sum(L * C * H * H for _n, C, H in spec.SITES) + (L - 1) * hw * (spec.GEN_CH + spec.DOWN_CH)) * 4
                rec.update(frac=6.0 * fl / avg / 1e9 / BF16_DENSE_PEAK_TFLOPS, frac_of=SPLIT_FRAC_OF,
                           fp32_equivalent_over_fp32_pipe_peak=fl / avg / 1e9 / MFMA_F32_PEAK_TFLOPS,
                           algorithmic_bytes=nbytes, achieved_gbs=nbytes / avg / 1e6, hbm_frac=nbytes / avg / 1e6 / HBM_PEAK_GBS)
        elif name.startswith("units:sobel S-blocks"):
            nbytes = P * hw * 4 * (spec.DOWN_CH + spec.DOWN_CH)          # read D, write S
            rec.update(bound="hbm", algorithmic_bytes=nbytes, achieved_gbs=nbytes / avg / 1e6,
                       frac=nbytes / avg / 1e6 / HBM_PEAK_GBS)
        elif name.startswith("units:sobel_tdiff"):
            nbytes = spec.algorithmic_bytes_sobel_tdiff(B, L)
            rec.update(bound="hbm", algorithmic_bytes=nbytes, achieved_gbs=nbytes / avg / 1e6,
                       frac=nbytes / avg / 1e6 / HBM_PEAK_GBS)
        elif "[winograd:" in name:
            # a conv on the Winograd path: the batched GEMMs against the fp32-MFMA peak with THEIR FLOPs (3x3 on 7x7 maps:
            # 2 * 121 * P * Ci * Co = 1 / 3.64 of the direct conv's), the two transforms against HBM with the bytes they move
            # (V written / M read; the map side is a fraction of that)
            key = name.split(" ")[0]
            co, ci, ksz = next((c, i, kk) for k_, c, i, kk, _s, _p in spec.FUSION_CONVS if k_ == key)
            T = 9 * P if ksz == 7 else P
            if "between]" in name:
                # wino_mid.hip: "<conv A> out + [<1x1 conv> +] <conv B> in": reads conv A's GEMM output M [121][P][Co_A], stores conv
                # A's activation where a later conv needs it (when a 1x1 conv sits in between) and writes conv B's GEMM input
                # V [121][P][Cmid]; the 1x1 conv's FLOPs ride along (0.6 / 2.5 GFLOP): bandwidth / latency bound
                parts = [q.strip().split(" ")[0] for q in name.split("[")[0].split("+")]
                mid_keys = parts[1:-1]
                cmid = next(c for k_, c, _i, _kk, _s, _p in spec.FUSION_CONVS if k_ == mid_keys[0]) if mid_keys else co
                nbytes = (121 * P * co + (P * 49 * co if mid_keys else 0) + 121 * P * cmid) * 4
                rec.update(bound="hbm", algorithmic_bytes=nbytes, achieved_gbs=nbytes / avg / 1e6, frac=nbytes / avg / 1e6 / HBM_PEAK_GBS)
                if mid_keys:
                    rec["flops_riding_along"] = work[mid_keys[0]]
                small_ms += avg
                small_fl += work[mid_keys[0]] if mid_keys else 0.0
            elif ksz == 7 and "GEMMs" not in name:
                # F(5x5, 4x4), four 14x14 phase images: 225 transformed floats per (tile, channel); 64 GEMM outputs per (tile, co)
                nbytes = (T * 225 * ci + P * 784 * ci) * 4 if "input" in name else (64 * T * co + P * 196 * co) * 4
                rec.update(bound="hbm", algorithmic_bytes=nbytes, achieved_gbs=nbytes / avg / 1e6, frac=nbytes / avg / 1e6 / HBM_PEAK_GBS)
            elif "GEMMs" in name:
                fl = winograd_gemm_flops(P, key)
                rec.update(bound="mfma", flops=fl, direct_conv_flops=work[key], achieved_tflops=fl / avg / 1e9, frac=fl / avg / 1e9 / peak)
                if precision == "f32split":      # wino_gemm_split_kernel: six bf16 plane products per fp32 product on the bf16 pipe
                    rec.update(frac=6.0 * fl / avg / 1e9 / BF16_DENSE_PEAK_TFLOPS, frac_of=SPLIT_FRAC_OF,
                               fp32_equivalent_over_fp32_pipe_peak=fl / avg / 1e9 / MFMA_F32_PEAK_TFLOPS)
                small_ms += avg if key not in big else 0.0
                small_fl += work[key] if key not in big else 0.0
            else:
                vpts = 400 * ci if ksz == 5 else 121 * ci          # transformed-input floats per image (polyphase: 400 phase-points)
                nbytes = (T * vpts + P * (196 if ksz == 5 else 49) * ci) * 4 if "input" in name else (121 * T * co + P * 49 * co) * 4
                rec.update(bound="hbm", algorithmic_bytes=nbytes, achieved_gbs=nbytes / avg / 1e6, frac=nbytes / avg / 1e6 / HBM_PEAK_GBS)
                small_ms += avg if key not in big else 0.0
        elif name in work or name.split(" ")[0] in work or name.startswith("chain_"):
            fl = work.get(name, work.get(name.split(" ")[0]))
            if fl is None:      # a fused bottleneck chain: "chain_<tag> = convA + convB + ..." (offk_api.hip)
                parts = [k.strip() for k in name.split("=", 1)[1].split("+")]
                fl = sum(work[k] for k in parts)
                cw = [k for k in parts if k in chain_winograd_convs(P, precision)]
                if cw:      # its 3x3 conv runs in Winograd form: frac stays on the direct-conv FLOPs (comparable across rounds), the executed ones beside it
                    rec["direct_conv_flops"] = fl
                    rec["executed_flops"] = fl - sum(work[k] - chain_winograd_flops(P) for k in cw)
            rec.update(bound="mfma", flops=fl, achieved_tflops=fl / avg / 1e9, frac=fl / avg / 1e9 / peak)
            if "executed_flops" in rec:
                rec["executed_frac"] = rec["executed_flops"] / avg / 1e9 / peak
            if precision == "f32split" and (name in SPLIT_1X1_LAUNCHES or (name.startswith("chain_") and split_chains(P, precision))):
                # the 1x1 convs on 7x7 maps (and chain 28a's branch conv) run in wino_gemm_split_kernel, the chains in chain14_split_kernel
                rec.update(frac=6.0 * fl / avg / 1e9 / BF16_DENSE_PEAK_TFLOPS, frac_of=SPLIT_FRAC_OF,
                           fp32_equivalent_over_fp32_pipe_peak=fl / avg / 1e9 / MFMA_F32_PEAK_TFLOPS)
            if name not in big:
                small_ms += avg
                small_fl += fl
        else:
            rec.update(bound="latency")
        kernels.append(rec)
    return {"precision": precision, "peak_tflops": peak, "steps": steps, "kernels": kernels,
            "small_conv_aggregate": {"avg_ms_per_forward": small_ms, "flops": small_fl,
                                     "frac": small_fl / small_ms / 1e9 / peak if small_ms > 0 else None,
                                     "what": "every fusion-stage launch except the 7x7, 5x5 and 3x3 832->256 convs"},
            "how": "offk_set_profiling(h, 2): HIP events on the forward's stream in front of every launch group, average "
                   "over the loop; frac = algorithmic FLOPs / time / peak (MFMA-bound) or algorithmic bytes / time / 8 TB/s"}


def dump_outputs(dirname, heads):
    """--dump-outputs: the three heads' scores (7, 14, 28) as DIR/logits_{7,14,28}.npy, float32."""
    os.makedirs(dirname, exist_ok=True)
    for name, t in zip(("logits_7", "logits_14", "logits_28"), heads):
        np.save(os.path.join(dirname, name + ".npy"), t.numpy().astype(np.float32))


def timed_loop(fn, steps, fence):
    fence()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    fence()
    return time.perf_counter() - t0


def units_training(B, L, variant, weights, feats, dev, precision, iters=10):
    """Secondary figure: train-mode forward of the nine units (dropout 0.8) and their
    backward (dM -> parameter gradients) at the bench size; random dM, same synthetic maps."""
    P = B * (L - 1)
    ht = runtime.OffForward(B, L, variant, spec.SLICE_FLAT, False, device=dev, precision=precision, training=True)
    ht.load_state_dict(weights)
    gen = torch.Generator(device=dev).manual_seed(5)
    bufs = [torch.randn(P, H, H, C, device=dev, generator=gen) for H, C in ((28, 320), (14, 1056), (7, 832))]
    views = [(bufs[0], 0), (bufs[0], 160)] + [(bufs[1], 160 * k) for k in range(5)] + [(bufs[2], 0), (bufs[2], 160)]
    grads = ht.new_unit_grads()

    def timed(fn):
        for _ in range(2):
            fn()
        return timed_loop(fn, iters, torch.cuda.synchronize) / iters * 1e3

    fwd = timed(lambda: ht.off_units_train(feats, 21, 0.8))
    bwd = timed(lambda: ht.off_units_backward(feats, views, 21, 0.8, grads=grads))
    hw = sum(H * H for _n, _c, H in spec.SITES)
    k2b = B * hw * 4 * ((160 + 32 + 32) * (L - 1) + 256 * L)
    k1b = sum(B * L * C * H * H * 4 for _n, C, H in spec.SITES) + B * hw * 4 * (128 * L + 32 * (L - 1))
    # a whole training step of the host-side module (off_module.OFFUnits): train-mode forward, backward into .grad, SGD
    # update, next forward sees the new weights -- the parameters are bound in place (offk_bind_weight), so the
    # "weight refresh" is the part of the step that no longer exists; measured here as the host time of OFFUnits._handle
    from offk_amd.off_module import OFFUnits
    units = OFFUnits(B, L, "rgb" if variant == spec.VARIANT_RGB else "flow", precision=precision).to(dev)
    units.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items() if k in units.state_dict()})
    units.train()
    opt = torch.optim.SGD([p_ for p_ in units.parameters() if p_.requires_grad], lr=1e-3)
    cots = [torch.randn(P, c, H, H, device=dev, generator=gen) for H, c in ((28, 320), (14, 800), (7, 320))]

    def train_step():
        opt.zero_grad(set_to_none=True)
        outs = units(feats, drop_seed=21)
        torch.autograd.backward(outs, cots)
        opt.step()

    step_ms = timed(train_step)
    params = [units._param(k) for k in units.param_keys]
    units._handle(dev, params)
    t0 = time.perf_counter()
    for _ in range(20):
        units._handle(dev, params)
    refresh_us = (time.perf_counter() - t0) / 20 * 1e6
    return {"precision": precision, "train_forward_ms": fwd, "backward_ms": bwd,
            "module_train_step_ms": step_ms,
            "module_train_step_note": "off_module.OFFUnits: forward (dropout 0.8) + backward + torch SGD step, wall clock; the "
                                      "three output copies and the permutes of the autograd boundary are inside",
            "weight_refresh_host_us_per_step": refresh_us,
            "weight_refresh_note": "unit parameters are bound in place (offk_bind_weight): after an optimizer step there is "
                                   "no copy, no packing kernel and no synchronisation; this is the host time of the per-step "
                                   "pointer check (54 tensors)",
            "clips_per_s_forward_plus_backward": B / (fwd + bwd) * 1e3,
            "backward_algorithmic_bytes": k2b + k1b, "backward_hbm_floor_ms_at_8TBs": (k2b + k1b) / 8e12 * 1e3,
            "note": "units only (K1+K2 train mode; K2b + weight-gradient GEMM + reductions); fusion stages / heads train on the caller's autograd"}


def split_error_vs_fp64(L, variant, weights, dev, kinds=("synth", "full_mantissa", "heavy_tail", "cancellation"), clips=2):
    """Both arithmetic modes of the units kernel (the one kernel with a split form so far) against an fp64 contraction of the same
    fp32 inputs (torch CPU, double): T = relu(G)[t + 1] - relu(G)[t] and D of all nine sites, RGB_OFF.py:597-610.  Per mode and
    input kind: max |err| / max |ref|, rms err / max |ref|, and the constant c of |err| <= c 2^-24 sum_k |w_k x_k| (max, rms).
    'cancellation': every channel of a pixel equal, every weight row zero-sum -- the exact result is the bias.  The same
    numbers are asserted in tests/test_gpu_split.py (split <= fp32 pipe on every one)."""
    import torch.nn.functional as F
    eps = 2.0 ** -24
    P = clips * (L - 1)

    def reference(feats_np, w):
        out = []
        for (name, _C, H), x in zip(spec.SITES, feats_np):
            xd = torch.from_numpy(x).double()
            wg, bg = torch.from_numpy(w["motion_conv_gen_%s.weight" % name]).double(), torch.from_numpy(w["motion_conv_gen_%s.bias" % name]).double()
            wd, bd = torch.from_numpy(w["motion_spatial_down_%s.weight" % name]).double(), torch.from_numpy(w["motion_spatial_down_%s.bias" % name]).double()
            G = torch.relu(F.conv2d(xd, wg, bg)).view(clips, L, 128, H, H)
            mG = (F.conv2d(xd.abs(), wg.abs()) + bg.abs().view(1, -1, 1, 1)).view(clips, L, 128, H, H)
            out.append(((G[:, 1:] - G[:, :-1]).reshape(P, 128, H, H), (mG[:, 1:] + mG[:, :-1]).reshape(P, 128, H, H),
                        F.conv2d(xd[:P], wd, bd), F.conv2d(xd[:P].abs(), wd.abs()) + bd.abs().view(1, -1, 1, 1)))
        return out

    def outputs(h):
        res = []
        for fkey, fd in spec.FUSION.items():
            width = 160 * len(fd["sites"]) + fd["carry"]
            buf = h.region("fusion_" + fkey, width).view(P, fd["H"], fd["H"], width)
            for i, sname in enumerate(fd["sites"]):
                res.append((buf[..., 160 * i + 32:160 * i + 160].permute(0, 3, 1, 2).double().cpu(),
                            h.region("D_" + sname, 32).view(P, fd["H"], fd["H"], 32).permute(0, 3, 1, 2).double().cpu()))
        return res

    table = {}
    for kind in kinds:
        w = dict(weights)
        if kind == "cancellation":
            for name, _C, _H in spec.SITES:
                for key in ("motion_conv_gen_%s.weight" % name, "motion_spatial_down_%s.weight" % name):
                    wk = w[key].astype(np.float64)
                    w[key] = (wk - wk.mean(axis=1, keepdims=True)).astype(np.float32)
            base = synth.make_features_kind(clips, L, 4, "heavy_tail")
            feats_np = [np.ascontiguousarray(np.broadcast_to(f[:, :1] + np.float32(0.5), f.shape)) for f in base]
        else:
            feats_np = synth.make_features_kind(clips, L, 4, kind)
        ref = reference(feats_np, w)
        feats = [torch.from_numpy(f).to(dev) for f in feats_np]
        for prec in ("fp32", "f32split"):
            h = runtime.OffForward(clips, L, variant, spec.SLICE_FLAT, False, device=dev, precision=prec)
            h.load_state_dict(w)
            h.off_units_fused(feats)
            torch.cuda.synchronize()
            mx = cmx = se = sc = 0.0
            n = 0
            for (T, D), (Tr, mT, Dr, mD) in zip(outputs(h), ref):
                for got, want, mag in ((T, Tr, mT), (D, Dr, mD)) if kind != "cancellation" else ((D, Dr, mD),):
                    e = (got - want).abs()
                    sN = want.abs().max().clamp_min(1e-30)
                    c = e / (mag.clamp_min(1e-30) * eps)
                    mx, cmx = max(mx, (e.max() / sN).item()), max(cmx, c.max().item())
                    se += ((e / sN) ** 2).sum().item()
                    sc += (c ** 2).sum().item()
                    n += e.numel()
            table.setdefault(prec, {})[kind] = {"max_over_max": mx, "rms_over_max": (se / n) ** 0.5, "c_max": cmx, "c_rms": (sc / n) ** 0.5}
            del h
    return table


def split_gemm_error_vs_fp64(dev, batch=6, M=384, K=832, Co=256):
    """Both forms of the batched GEMMs of the Winograd convs (offk_batched_gemm_nt: wino_gemm.hip on the fp32 pipe, wino_gemm_split.hip
    in split-fp32) against an fp64 contraction of the same fp32 inputs, at the shape of motion_conv_trans's GEMMs (K = 832, Co = 256,
    384 rows per point): the four numbers of split_error_vs_fp64 per mode and input kind.  Asserted in tests/test_gpu_split.py."""
    eps = 2.0 ** -24
    table = {}
    for kind in ("relu", "normal", "heavy_tail", "cancellation"):
        g = torch.Generator().manual_seed(5)
        x = torch.randn(batch, M, K, generator=g)
        w = torch.randn(batch, Co, K, generator=g) * (1.0 / K ** 0.5)
        if kind == "relu":
            x = torch.relu(x)
        elif kind == "heavy_tail":
            x = x * torch.exp(2.0 * torch.randn(batch, M, 1, generator=g))
        elif kind == "cancellation":
            w = w - w.mean(dim=2, keepdim=True)
            x = 3.0 + torch.randn(batch, M, 1, generator=g) + torch.randn(batch, M, K, generator=g) * 2.0 ** -12
        x, w = x.float().contiguous(), w.float().contiguous()
        ref = torch.einsum("bmk,bnk->bmn", x.double(), w.double())
        mag = torch.einsum("bmk,bnk->bmn", x.double().abs(), w.double().abs())
        for prec in ("fp32", "f32split"):
            y = runtime.batched_gemm_nt(x.to(dev), w.to(dev), prec).double().cpu()
            e = (y - ref).abs()
            c = e / (mag.clamp_min(1e-30) * eps)
            sN = ref.abs().max()
            table.setdefault(prec, {})[kind] = {"max_over_max": (e.max() / sN).item(), "rms_over_max": ((e / sN) ** 2).mean().sqrt().item(),
                                                "c_max": c.max().item(), "c_rms": (c ** 2).mean().sqrt().item()}
    return table


def split_vs_fp32_forward(B, L, variant, weights, dev, kinds=("synth", "full_mantissa", "heavy_tail"), clips=8):
    """The whole forward in both modes on the same inputs: max |diff| / max |fp32-mode value| over the three logit tensors and sum_7."""
    out, hs = {}, {}
    for prec in ("fp32", "f32split"):
        hs[prec] = runtime.OffForward(clips, L, variant, spec.SLICE_FLAT, False, device=dev, precision=prec)
        hs[prec].load_state_dict(weights)
    for kind in kinds:
        feats = [torch.from_numpy(f).to(dev) for f in synth.make_features_kind(clips, L, 2, kind)]
        res = {}
        for prec, h in hs.items():
            o = h.forward(feats)
            res[prec] = [t.double() for t in o] + [h.region("sum_7", 1024).double().clone()]
        torch.cuda.synchronize()
        errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(res["f32split"], res["fp32"])]
        out[kind] = {"logits": max(errs[:3]), "sum_7": errs[3]}
    return out


def flow_variant(B, L, dev, steps, warmup, measure, precision):
    """BASELINE config 3: Flow_OFF forward (Flow_OFF.py:606-876), batch = 64, consensus inside, in the headline's arithmetic."""
    w = synth.make_weights(spec.VARIANT_FLOW)
    f = [torch.from_numpy(x).to(dev) for x in synth.make_features(B, L, config_id=3)]
    h, dt, _s, _k = measure(precision, steps, warmup, variant=spec.VARIANT_FLOW, weights=w, feats=f, consensus=True, k2=False)
    del h
    return {"workload": "Flow_OFF forward (fixed diagonal Sobel, SegmentConsensus avg), batch=%d clips x %d segments" % (B, L),
            "value": B * steps / dt, "unit": "clips/s", "ms_per_step": dt / steps * 1e3, "steps": steps, "warmup": warmup,
            "precision": precision, "dtype": DTYPES[precision]}


def two_stream_leg(B, L, dev, steps, warmup, rgb_feats, rgb_weights, precision):
    """BASELINE config 5, the per-GPU leg: RGB-OFF and Flow-OFF forwards of the same clips on two HIP streams, then K7
    (offk_score_fusion) over the six score sets with the notebook's weights (score_fusion.ipynb lines 300-301)."""
    from offk_amd import two_stream
    ts = two_stream.TwoStreamOFF(B, L, precision=precision, device=dev)
    ts.load_state_dicts(rgb_weights, synth.make_weights(spec.VARIANT_FLOW, seed=0xF10))
    ff = [torch.from_numpy(x).to(dev) for x in synth.make_features(B, L, config_id=3)]
    tsn_r = torch.from_numpy(synth.uniform_values(0x7501, B * spec.NUM_CLASSES, 4.0).reshape(B, -1)).to(dev)
    tsn_f = torch.from_numpy(synth.uniform_values(0x7502, B * spec.NUM_CLASSES, 4.0).reshape(B, -1)).to(dev)

    def step():
        ts.forward(rgb_feats, ff, rgb_tsn=tsn_r, flow_tsn=tsn_f)

    for _ in range(warmup):
        step()
    dt = timed_loop(step, steps, torch.cuda.synchronize)
    return {"workload": "RGB_OFF + Flow_OFF forwards of the same %d clips x %d segments on two HIP streams + K7 late fusion "
                        "(6 score sets incl. both TSN scores) + argmax" % (B, L),
            "value": B * steps / dt, "unit": "clips/s (a clip = both streams)", "ms_per_step": dt / steps * 1e3,
            "steps": steps, "warmup": warmup, "precision": precision, "dtype": DTYPES[precision]}


@contextlib.contextmanager
def stdout_to_stderr():
    """fd 1 -> fd 2 while a communicator is created: gloo's "[Gloo] Rank ..." and RCCL's "RCCL version : ..." banners are
    written by C++ code on fd 1, and stdout is for the one JSON line."""
    sys.stdout.flush()
    saved = os.dup(1)
    os.dup2(2, 1)
    try:
        yield
    finally:
        sys.stdout.flush()
        os.dup2(saved, 1)
        os.close(saved)


def init_single_rank_rccl(dev):
    """A world_size-1 RCCL ("nccl" backend on ROCm) process group in THIS process: no launcher, no re-exec after the GPU is
    initialised.  Rendezvous over a loopback TCP store on a free port."""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("nccl", init_method="tcp://127.0.0.1:%d" % port, rank=0, world_size=1, device_id=dev)


def rccl_smoke_object(B, L, variant, weights, feats, dev, steps, precision, form_used):
    """Secondary object of the default N = 1 line: the per-step score exchange of config 4 executed on RCCL with a single-rank group on the
    one GPU of the box -- librccl init, then EACH form of the exchange alone behind a consensus forward (the real N > 1 step issues one of
    them): `all_gather_into_tensor`, and the zero-buffer `all_reduce`, both through offk_amd.dist, asynchronous (two alternating buffer
    sets) and, for comparison with rounds <= 4, synchronous.  NOT a scaling number.  Failures are recorded, not raised: the headline
    measurement does not depend on RCCL."""
    rec = {"what": "single-rank RCCL smoke, not a scaling number", "world_size": 1, "precision": precision}
    try:
        if not dist.is_initialized():
            with stdout_to_stderr():      # (device_id = eager communicator: RCCL's banner comes with the init)
                init_single_rank_rccl(dev)
        rec["backend"] = dist.get_backend()
        h = runtime.OffForward(B, L, variant, spec.SLICE_FLAT, True, device=dev, precision=precision)
        h.load_state_dict(weights)
        arr = h._feat_array(feats)
        ncls = spec.NUM_CLASSES
        local = [torch.empty(3, B, ncls, device=dev) for _ in range(2)]
        gathered = [torch.empty(1, 3, B, ncls, device=dev) for _ in range(2)]
        xg = odist.ScoreExchange(2)
        cnt = [0]

        def make_step(form, asynchronous):
            def step():
                i = cnt[0] & 1
                cnt[0] += 1
                xg.wait_slot(i)
                h.forward_into(arr, local[i][0], local[i][1], local[i][2])
                if form == "allgather":
                    if asynchronous:
                        xg.all_gather(i, gathered[i], local[i])
                    else:
                        odist.all_gather_scores_into(gathered[i], local[i])
                elif form == "allreduce":     # world_size 1: this rank's rows ARE the zeroed [head][world * rows][class] buffer
                    if asynchronous:
                        xg.all_reduce(i, local[i])
                    else:
                        odist.all_reduce_scores_inplace(local[i])
            return step

        def fence():
            xg.finish()
            torch.cuda.synchronize()
            dist.barrier()
            torch.cuda.synchronize()

        with stdout_to_stderr():      # the first collective creates the communicator
            for form in ("allgather", "allreduce"):
                st = make_step(form, True)
                for _ in range(3):
                    st()
            fence()
        times = {}
        for rep in range(2):          # two interleaved passes, the smaller of each: the differences are tens of microseconds
            for key, form, asyn in (("plain", None, True), ("allgather", "allgather", True), ("allreduce", "allreduce", True),
                                    ("allgather_sync", "allgather", False), ("allreduce_sync", "allreduce", False)):
                t = timed_loop(make_step(form, asyn), steps, fence) / steps * 1e3
                times[key] = min(times.get(key, t), t)
        # correctness of both forms on the buffers of one more step each
        make_step("allgather", True)()
        fence()
        last = (cnt[0] - 1) & 1
        ok = bool(torch.equal(gathered[last][0], local[last]))
        want = local[last].clone()
        xg.all_reduce(last, local[last])
        fence()
        ok = ok and bool(torch.equal(local[last], want))
        rec.update(ms_per_step_without_exchange=times["plain"], ms_per_step_allgather=times["allgather"], ms_per_step_allreduce=times["allreduce"],
                   allgather_us_per_step=(times["allgather"] - times["plain"]) * 1e3,
                   allreduce_us_per_step=(times["allreduce"] - times["plain"]) * 1e3,
                   allgather_sync_us_per_step=(times["allgather_sync"] - times["plain"]) * 1e3,
                   allreduce_sync_us_per_step=(times["allreduce_sync"] - times["plain"]) * 1e3,
                   form_used_by_gpus_N=form_used, mode="async_op=True, two alternating buffer sets (sync variants beside it in the detail file)",
                   steps=steps, n_ranks_seen=dist.get_world_size(), exchange_ok=ok,
                   per_step="consensus forward + ONE form of the exchange of the [3 heads][B][101] scores; each loop fenced by barrier + synchronize; "
                            "min of two interleaved passes")
    except Exception as e:      # noqa: BLE001 -- a broken RCCL install must not take the headline line with it
        rec["error"] = "%s: %s" % (type(e).__name__, e)
    return rec


LINE_LIMIT = 8192        # the driver keeps the last 8 KB of stdout: the one line must fit with room to spare (BENCH_r05: 22 KB -> parsed null)
LINE_TARGET = 6000


def _sig(x, n=5):
    """Floats to n significant digits (the line is for reading and parsing, bench_detail.json keeps every digit)."""
    if isinstance(x, bool) or not isinstance(x, float):
        return x
    if x != x or x in (float("inf"), float("-inf")):
        return None
    return float("%.*g" % (n, x))


def _pick(d, keys):
    return dict((k, _sig(d[k])) for k in keys if isinstance(d, dict) and k in d)


def _worst(table, mode):
    """error table {mode: {kind: {max_over_max, rms_over_max, c_max, c_rms}}} -> the worst max_over_max / c_max of a mode over the
    non-cancellation kinds (the cancellation case is normalised by the output, not by the contraction: its own pair beside it)."""
    rows = (table or {}).get(mode)
    if not rows:
        return None
    plain = [v for k, v in rows.items() if k != "cancellation"] or list(rows.values())
    out = {"max_over_max": _sig(max(v["max_over_max"] for v in plain), 3), "c_max": _sig(max(v["c_max"] for v in plain), 3)}
    if "cancellation" in rows:
        out["cancellation_c_max"] = _sig(rows["cancellation"]["c_max"], 3)
    return out


def _mode_object(full, mode):
    """The compact per-mode object: value, ms_per_step, dtype, the units kernel's time and fraction, the mode's worst error against fp64."""
    src = full if full.get("precision") == mode else full.get(("fp32_pipe" if mode == "fp32" else mode) + "_mode")
    if not isinstance(src, dict):
        return None
    rec = _pick(src, ("value", "ms_per_step", "steps"))
    rec["dtype"] = "f32 on v_mfma_f32_* (fp32 pipe)" if mode == "fp32" else "f32 as 3 bf16 planes x 6 exact products, f32 accumulate (bf16 pipe)"
    uk = src.get("units_kernel")
    if isinstance(uk, dict):
        rec["units_kernel"] = {"us": _sig(uk["avg_ms"] * 1e3, 4), "frac": _sig(uk.get("frac"), 3),
                               "of": "2.5 PF bf16 (6 products per fp32 product)" if mode == "f32split" else "157.3 TF fp32 MFMA"}
        if "hbm_frac" in uk:
            rec["units_kernel"]["hbm_frac"] = _sig(uk["hbm_frac"], 3)
    e = _worst(full.get("error_vs_fp64"), mode)
    if e:
        rec["units_error_vs_fp64"] = e
    e = _worst(full.get("gemm_error_vs_fp64"), mode)
    if e:
        rec["gemm_error_vs_fp64"] = e
    if full.get("precision") == mode:
        rec["headline"] = True
    return rec


def compact_line(full, detail_path=None):
    """The ONE stdout line: what the driver parses (metric / value / ms_per_step / dtype / config / roofline / cpu_baseline) plus one small
    object per secondary measurement.  `full` is the complete result object main() builds (-> bench_detail.json).  Always < LINE_LIMIT:
    optional objects are dropped, last first, should it ever grow past LINE_TARGET."""
    line = _pick(full, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                        "vs_baseline", "dtype", "data"))
    line["config"] = _pick(full.get("config", {}), ("workload", "global_batch", "segments", "parallelism", "slice_mode", "arithmetic"))
    line.update(_pick(full, ("n_ranks_seen", "collective_backend", "exchange_ok", "exchange")))
    rf = full.get("roofline")
    if isinstance(rf, dict):
        r = _pick(rf, ("bound", "kernel", "achieved", "peak", "unit", "frac", "traffic", "algorithmic_bytes_per_launch", "avg_launch_us",
                       "min_launch_us", "launches", "on_default_forward_path"))
        if isinstance(rf.get("in_path"), dict):
            r["in_path"] = _pick(rf["in_path"], ("kernel", "achieved", "frac", "avg_launch_us", "algorithmic_bytes_per_launch"))
        line["roofline"] = r
    ip = full.get("roofline_in_path")
    if isinstance(ip, dict):
        o = {}
        if isinstance(ip.get("dominant"), dict):
            o["dominant"] = _pick(ip["dominant"], ("launch", "avg_ms", "bound", "frac", "frac_of", "hbm_frac", "share_of_step"))
        top = sorted((k for k in ip.get("kernels", []) if "avg_ms" in k), key=lambda k: -k["avg_ms"])[:6]
        o["top_launches"] = [[k["launch"][:48], _sig(k["avg_ms"] * 1e3, 4), ("bf16-mfma" if "frac_of" in k else k.get("bound")), _sig(k.get("frac"), 3)]
                             for k in top]
        o["top_launches_columns"] = ["launch", "us", "bound (mfma = 157.3 TF fp32 pipe, bf16-mfma = 6 products / 2.5 PF, hbm = 8 TB/s)", "frac of that peak"]
        o["n_launch_groups"] = len(ip.get("kernels", []))
        line["roofline_in_path"] = o
    if isinstance(full.get("mfma"), dict):
        line["mfma"] = _pick(full["mfma"], ("peak_tflops", "executed_flops_per_step", "executed_frac_of_peak", "executed_frac_is"))
    cb = full.get("cpu_baseline")
    if isinstance(cb, dict):
        c = _pick(cb, ("value", "unit", "cores", "cpu_model", "kind", "sample", "usable_cpus", "host_logical_cpus"))
        c["operating_points_clips_per_s"] = dict((k, _sig(cb[k]["value"], 4)) for k in ("batch_1", "batch_large", "concurrent_batch_1")
                                                 if isinstance(cb.get(k), dict))
        line["cpu_baseline"] = c
        line["gpu_over_cpu"] = _sig(full.get("gpu_over_cpu"))
    for mode, key in (("f32split", "f32split_mode"), ("fp32", "fp32_pipe_mode")):
        m = _mode_object(full, mode)
        if m:
            line[key] = m
    if isinstance(full.get("max_rel_diff_between_modes"), dict):
        d = full["max_rel_diff_between_modes"]
        line["max_rel_diff_between_modes"] = {"logits": _sig(max(v["logits"] for v in d.values()), 3),
                                              "sum_7": _sig(max(v["sum_7"] for v in d.values()), 3)}
    optional = []
    for key in ("flow_variant", "two_stream"):
        if isinstance(full.get(key), dict):
            line[key] = _pick(full[key], ("value", "ms_per_step", "precision"))
            optional.append(key)
    sm = full.get("rccl_single_rank_smoke")
    if isinstance(sm, dict):
        line["rccl_single_rank_smoke"] = _pick(sm, ("backend", "n_ranks_seen", "exchange_ok", "ms_per_step_without_exchange", "allgather_us_per_step",
                                                    "allreduce_us_per_step", "form_used_by_gpus_N", "mode", "error"))
        optional.append("rccl_single_rank_smoke")
    for key in ("single_rank_rccl_smoke", "oversubscribed"):
        if isinstance(full.get(key), dict):
            line[key] = _pick(full[key], ("backend", "world_size", "ranks", "gpus_visible", "note"))
    if detail_path:
        line["detail"] = detail_path
    for key in reversed(optional + ["max_rel_diff_between_modes", "mfma"]):
        if len(json.dumps(line)) <= LINE_TARGET:
            break
        line.pop(key, None)
    if len(json.dumps(line)) >= LINE_LIMIT:      # cannot happen with the fields above; never hand the driver an unparseable line
        for key in ("roofline_in_path", "fp32_pipe_mode", "f32split_mode"):
            line.pop(key, None)
    return line


def emit(full, detail_path):
    """Rank 0: full object -> detail file + stderr, compact object -> the one stdout line (last thing written)."""
    where = None
    try:
        with open(detail_path, "w") as f:
            json.dump(full, f, indent=1)
        where = os.path.relpath(detail_path, ROOT) if detail_path.startswith(ROOT) else detail_path
    except OSError as e:
        sys.stderr.write("bench.py: could not write %s (%s); the full object follows on stderr only\n" % (detail_path, e))
    sys.stderr.write("bench.py full result object (also %s):\n%s\n" % (where, json.dumps(full)))
    sys.stderr.flush()
    text = json.dumps(compact_line(full, where))
    assert len(text) < LINE_LIMIT, len(text)
    sys.stdout.write(text + "\n")
    sys.stdout.flush()


def main():
    args = ARGS
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        args.gpus = world          # under a launcher the launcher's world size is authoritative
    over = bool(args.oversubscribe) and world > 1
    ndev = torch.cuda.device_count()
    dev_index = local_rank % max(ndev, 1) if over else local_rank
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    backend = None
    smoke = bool(args.collective_smoke) and world == 1
    if smoke:
        with stdout_to_stderr():
            init_single_rank_rccl(dev)
        backend = dist.get_backend()
    coll = world > 1 or smoke            # the step ends with the score exchange
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if over:    # several ranks per device: RCCL refuses that, the scores travel over gloo (host-staged)
            with stdout_to_stderr():
                dist.init_process_group("gloo", rank=rank, world_size=world)
                dist.barrier()
        else:
            with stdout_to_stderr():      # (the communicator, and RCCL's banner with it, comes with the first collective)
                dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)
                dist.barrier()
                torch.cuda.synchronize()
        backend = dist.get_backend()

    variant = spec.VARIANT_RGB if args.variant == "rgb" else spec.VARIANT_FLOW
    B, L = args.batch, args.length
    consensus = (variant == spec.VARIANT_FLOW) or coll
    weights = synth.make_weights(variant)
    feats_np = make_features(B, L, config_id=2, clip_offset=rank * B)
    feats = [torch.from_numpy(f).to(dev) for f in feats_np]
    rows = B if consensus else B * (L - 1)
    ncls = spec.NUM_CLASSES
    out = [torch.empty(rows, ncls, device=dev) for _ in range(3)]
    # two buffer sets, alternated per step: the collective of step i (RCCL stream) may still be reading
    # its input while the forward of step i+1 is enqueued on the compute stream
    gathered = local = reduced = None
    if coll and (args.collective == "allgather" or smoke):
        gathered = [torch.empty(world, 3, rows, ncls, device=dev) for _ in range(2)]
        local = [torch.empty(3, rows, ncls, device=dev) for _ in range(2)]
    if coll and (args.collective == "allreduce" or smoke):
        # all-reduce form: this rank's rows of a zeroed [head][world * rows][class] buffer + one sum
        reduced = [torch.zeros(3, world * rows, ncls, device=dev) for _ in range(2)]
        if local is None:     # the forward writes straight into its rows of the buffer
            local = [g[:, rank * rows:(rank + 1) * rows] for g in reduced]
    last_exchange = [None, 0]
    # the exchange runs asynchronously (dist.ScoreExchange): the compute stream is not ordered behind the collective of the step before;
    # a buffer set is waited for when it comes round again (two steps later), everything outstanding at the fences
    xchg, xchg2 = odist.ScoreExchange(2), odist.ScoreExchange(2)

    def fence():
        xchg.finish()
        xchg2.finish()
        torch.cuda.synchronize()
        if coll:
            dist.barrier()
        torch.cuda.synchronize()

    def exchange(i):
        """config 4: the only exchange on the path -- per-clip consensus scores, one collective per step."""
        last_exchange[1] = i
        if over:      # host-staged over gloo: the same offk_amd.dist calls tests/test_dist_gloo.py pins
            mine = torch.stack([local[i][k] for k in range(3)], 0).cpu()
            fn = odist.gather_scores if args.collective == "allgather" else odist.gather_scores_allreduce
            last_exchange[0] = fn(mine)
        elif smoke:       # single-rank RCCL group: BOTH forms of the exchange, every step
            xchg.all_gather(i, gathered[i], local[i])
            reduced[i].zero_()
            reduced[i][:, rank * rows:(rank + 1) * rows] = local[i]
            xchg2.all_reduce(i, reduced[i])
            last_exchange[0] = gathered[i]
        elif args.collective == "allgather":
            xchg.all_gather(i, gathered[i], local[i])
            last_exchange[0] = gathered[i]
        else:
            xchg.all_reduce(i, reduced[i])
            last_exchange[0] = reduced[i]

    def exchanged():
        """The scores the last exchange delivered, on the host: [head][rank * rows + row][class]."""
        got = last_exchange[0]
        if torch.is_tensor(got) and got.dim() == 4:      # all-gather layout [rank][head][row] -> [head][rank * rows + row]
            got = got.view(world, 3, rows, ncls).permute(1, 0, 2, 3).reshape(3, world * rows, ncls)
        return got.cpu()

    def measure(precision, steps, warmup, variant=variant, weights=weights, feats=feats, consensus=consensus, k2=True, dump=None):
        """W untimed steps, K timed steps between fences (profiling off), the last step's outputs to `dump` (--dump-outputs), then
        with --full a second loop of K steps with the library's per-stage HIP events on and a standalone K2 launch (the roofline
        object) after every forward."""
        h = runtime.OffForward(B, L, variant, spec.SLICE_FLAT, consensus, device=dev, precision=precision)
        h.load_state_dict(weights)
        arr = h._feat_array(feats)
        counter = [0]

        def step():
            if coll:
                i = counter[0] & 1
                counter[0] += 1
                xchg.wait_slot(i)             # the collective that used this buffer set two steps ago
                xchg2.wait_slot(i)
                if args.collective == "allreduce" and not smoke:
                    reduced[i].zero_()
                h.forward_into(arr, local[i][0], local[i][1], local[i][2])
                exchange(i)
            else:
                h.forward_into(arr, out[0], out[1], out[2])

        for _ in range(warmup):
            step()
        dt = timed_loop(step, steps, fence)
        if world > 1:
            t = torch.tensor([dt], device="cpu" if over else dev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = t.item()
        if dump and rank == 0:
            dump_outputs(dump, exchanged() if coll else [o.cpu() for o in out])
        if not (k2 and args.full):
            return h, dt, None, None
        # second loop: where the time goes, and K2 on its own (HIP events on the stream the kernels run on)
        h.off_units(feats)                      # G / D regions hold real data whichever units path the forward takes
        h.set_profiling(True)
        h.stage_times(reset=True)
        k2_ev = []
        for _ in range(steps):
            h.forward_into(arr, out[0], out[1], out[2]) if not coll else step()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K2_PER_PAIR):
                h.sobel_tdiff_all(0)
            e1.record()
            k2_ev.append((e0, e1))
        torch.cuda.synchronize()
        stages = h.stage_times(reset=True)
        h.set_profiling(False)
        k2_us = [a.elapsed_time(b) * 1e3 / K2_PER_PAIR for a, b in k2_ev]
        return h, dt, stages, k2_us

    h, dt, stages, k2_us = measure(args.precision, args.steps, args.warmup, dump=args.dump_outputs)
    in_path = roofline_in_path(h, h._feat_array(feats), out, B, L, args.precision, min(args.steps, 20)) if world == 1 and args.full else None
    # With an exchange on the step: the exchanged scores must hold EVERY rank's shard in clip order.  Checked once, outside the timed
    # region, against an independent reference: one more forward + exchange, this rank's rows cloned BEFORE the collective (in the
    # all-reduce form `local` is a view of the buffer being reduced), the clones of all ranks gathered by a second, plain collective.
    exchange_ok = None
    if coll and args.full:
        i_chk = 0
        xchg.finish()
        xchg2.finish()
        if reduced is not None and not smoke and args.collective == "allreduce":
            reduced[i_chk].zero_()
        h.forward_into(h._feat_array(feats), local[i_chk][0], local[i_chk][1], local[i_chk][2])
        torch.cuda.synchronize()
        mine = torch.stack([local[i_chk][k] for k in range(3)], 0).clone()
        exchange(i_chk)
        xchg.finish()
        xchg2.finish()
        torch.cuda.synchronize()
        got = exchanged()
        ref_parts = [torch.empty_like(mine.cpu() if over else mine) for _ in range(world)]
        dist.all_gather(ref_parts, mine.cpu() if over else mine)
        ref = torch.cat([r_.cpu() for r_ in ref_parts], 1)
        good = tuple(got.shape) == (3, world * rows, ncls) and bool(torch.isfinite(got).all()) and torch.equal(got, ref)
        if smoke:       # ... and the all-reduce form of the same step
            good = good and torch.equal(reduced[i_chk].cpu(), ref)
        for r in range(world):      # the shards are different clips: no two ranks may hold the same rows
            if r != rank:
                good = good and not torch.equal(ref[:, r * rows:(r + 1) * rows], mine.cpu())
        if args.dump_scores and rank == 0:
            np.save(args.dump_scores, got.numpy())
        ok = torch.tensor([1.0 if good else 0.0], device="cpu" if over else dev)
        dist.all_reduce(ok, op=dist.ReduceOp.MIN)
        exchange_ok = bool(ok.item() == 1.0)

    if rank == 0:
        ms_step = dt / args.steps * 1e3
        clips_s = world * B * args.steps / dt
        if not coll:
            coll_txt = ""
        elif smoke:
            coll_txt = (" + SegmentConsensus avg + SINGLE-RANK RCCL SMOKE (world_size 1 on the one GPU of this box: librccl init, "
                        "all_gather_into_tensor and the zero-buffer all_reduce form of the per-clip score exchange inside every "
                        "timed step; not a scaling number)")
        elif over:
            coll_txt = " + SegmentConsensus avg + %s of per-clip scores over gloo (host-staged; OVERSUBSCRIBED: %d ranks on %d GPU(s))" % (
                args.collective, world, ndev)
        else:
            coll_txt = " + SegmentConsensus avg + RCCL %s of per-clip scores" % args.collective
        wino_on = os.environ.get("OFFK_WINOGRAD", "1") != "0"
        res = {
            "metric": "OFF-forward clips/sec (7-seg 224x224)", "value": clips_s, "unit": "clips/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": DTYPES[args.precision], "precision": args.precision,
            "data": "synthetic (portable counter-based generator: ReLU-like non-negative BN-Inception "
                    "feature maps, fan-in-scaled uniform weights; features resident in HBM)",
            "config": {"workload": "%s_OFF forward, batch=%d clips/GPU x %d segments, nine 224x224-geometry "
                                   "feature maps%s" % (args.variant.upper(), B, L, coll_txt),
                       "global_batch": world * B, "segments": L, "parallelism": "clip-shard x%d" % world,
                       "slice_mode": "reference_flat",
                       "arithmetic": ("fp32 MFMA products, fp32 accumulation" if args.precision == "fp32" else
                                      "split-fp32 (three bf16 planes per fp32 operand, six exact plane products on the bf16 pipe, fp32 accumulation) in the "
                                      "units kernel, the Winograd GEMMs, the bottleneck chains and every 1x1 conv on 7x7 maps (no MFMA-bound launch of this mode is left "
                                      "on the fp32 pipe)") +
                                     ("; the k x k fusion convs in Winograd forms (fp32 transforms)" if wino_on else "; direct convolutions")},
            "n_ranks_seen": dist.get_world_size() if coll else 1, "collective_backend": backend,
            "exchange": ("async_op=True on two alternating buffer sets: the timed step does not wait for its own collective, only the "
                         "closing fence does (round 5 on; earlier rounds' multi-rank ms_per_step had it inside every step)") if coll else None,
        }
        if args.full:
            k2_avg_s = sum(k2_us) / len(k2_us) * 1e-6
            algo_bytes = spec.algorithmic_bytes_sobel_tdiff(B, L)
            achieved = algo_bytes / k2_avg_s / 1e9
            unit_f, fus_f = spec.flops_per_clip(L)
            stage_ms = dict((k, v[0] / max(v[1], 1)) for k, v in stages.items())
            gpu_ms = sum(stage_ms.values())
            peak_tf = MFMA_F32_PEAK_TFLOPS
            algo_flops = (unit_f + fus_f) * B                  # per rank; ms_step is a rank's time: the fractions below are per GPU
            exec_flops = algo_flops - winograd_saved_flops(B * (L - 1), args.precision) if wino_on else algo_flops
            s_blocks = next((k for k in (in_path or {}).get("kernels", []) if k["launch"].startswith("units:sobel S-blocks")), None)
            res.update({
                "roofline": {"bound": "hbm", "kernel": "sobel_tdiff_kernel (K2: temporal difference + spatial gradient + concat, "
                                                       "all nine sites, one launch; offk_sobel_tdiff_all)",
                             "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": achieved / HBM_PEAK_GBS, "traffic": measured_traffic(B, L, args.variant),
                             "algorithmic_bytes_per_launch": algo_bytes, "avg_launch_us": k2_avg_s * 1e6,
                             "min_launch_us": min(k2_us), "launches": len(k2_us) * K2_PER_PAIR,
                             "on_default_forward_path": False,
                             "in_path": None if s_blocks is None else {
                                 "kernel": "sobel_tdiff_kernel<..., ROLES = 3> (the S-blocks: read D, depthwise 3x3 / diagonal Sobel, write S)",
                                 "achieved": s_blocks["achieved_gbs"], "frac": s_blocks["frac"], "avg_launch_us": s_blocks["avg_ms"] * 1e3,
                                 "algorithmic_bytes_per_launch": s_blocks["algorithmic_bytes"]},
                             "quote_as": "%.2f of 8 TB/s standalone (the whole Sobel + temporal-difference kernel) / %s in path (its S-blocks, "
                                         "the part the timed forward launches)" % (achieved / HBM_PEAK_GBS,
                                                                                   "n/a" if s_blocks is None else "%.2f" % s_blocks["frac"]),
                             "path_note": "the north-star object (Sobel + temporal-diff kernel) launched STANDALONE: the default "
                                          "inference forward fuses the temporal difference into the 1x1 reduce (pw_tdiff, MFMA-bound) "
                                          "and runs only this kernel's S-blocks; the full kernel serves training and "
                                          "OFFK_FUSED_UNITS=0.  What bounds the kernels the timed forward launches: roofline_in_path",
                             "how": "%d standalone launches between one HIP-event pair on the forward's stream, after every "
                                    "forward of a second K-step loop (the wall-clock loop runs without any event); an event "
                                    "pair around a single launch adds ~5 us of command-processor time to this kernel -- "
                                    "rocprofv3's kernel-trace average (profiles/) is the cross-check" % K2_PER_PAIR},
                "stage_ms": stage_ms,
                "mfma": {"peak_tflops": peak_tf,
                         "executed_flops_per_step": exec_flops,
                         "executed_frac_of_peak": exec_flops / (ms_step * 1e-3) / 1e12 / peak_tf,
                         "executed_frac_is": "fp32-equivalent FLOPs the matrix pipes execute (direct-conv FLOPs minus what the Winograd forms save) / "
                                             "wall-clock ms_per_step / the fp32 MFMA peak 157.3 TF, per GPU" +
                                             ("; in split-fp32 mode the units kernel, the Winograd GEMMs and the 7x7-map 1x1 convs run six bf16 plane "
                                              "products per fp32 product on the 2.5 PF bf16 pipe, so this is a throughput-equivalent there, "
                                              "not a utilisation" if args.precision == "f32split" else ""),
                         "algorithmic_flops_per_step": algo_flops,
                         "algorithmic_flops_over_peak": algo_flops / (ms_step * 1e-3) / 1e12 / peak_tf,
                         "algorithmic_tflops_over_summed_stage_time": algo_flops / (gpu_ms * 1e-3) / 1e12 if gpu_ms > 0 else 0.0,
                         "note": "the Winograd forms: the 3x3 / stride 1 convs on 7x7 maps run 1 / 3.64 of their multiplies, the polyphase 5x5 / "
                                 "stride 2 conv 1 / 3.06, the polyphase 7x7 / stride 2 conv 1 / 4.7, the 3x3 inside a bottleneck chain 1 / 2.25.  "
                                 "algorithmic_flops_over_peak counts DIRECT-convolution FLOPs instead: a throughput-equivalent, NOT a "
                                 "utilisation -- it can exceed 1 under Winograd."},
            })
        if in_path is not None:
            dom = max((k for k in in_path["kernels"] if "frac" in k), key=lambda k: k["avg_ms"], default=None)
            if dom is not None:
                in_path["dominant"] = {"launch": dom["launch"], "avg_ms": dom["avg_ms"], "bound": dom["bound"], "frac": dom["frac"],
                                       "share_of_step": dom["avg_ms"] / ms_step}
            res["roofline_in_path"] = in_path
            res["units_kernel"] = next((k for k in in_path["kernels"] if k["launch"].startswith("units:pw_tdiff")), None)
        if coll:
            res["exchange_ok"] = exchange_ok
            if smoke:
                res["single_rank_rccl_smoke"] = {"backend": backend, "world_size": dist.get_world_size(),
                                                 "per_step": "forward + all_gather_into_tensor + zero-buffer all_reduce (dist.py)",
                                                 "note": "NOT a scaling number: executes librccl (init + both collectives) on the one GPU there is"}
            if over:
                res["oversubscribed"] = {"ranks": world, "gpus_visible": ndev,
                                         "note": "NOT a scaling number: %d ranks time-share %d GPU(s); this run exists to execute "
                                                 "the multi-rank code path (clip_offset sharding, alternating buffers, the score "
                                                 "exchange, max-over-ranks timing) on hardware" % (world, ndev)}
        if args.full and world == 1 and not args.no_secondary:
            other = "f32split" if args.precision == "fp32" else "fp32"
            _h2, dt2, st2, _k2 = measure(other, args.steps, args.warmup)
            sec = {"value": B * args.steps / dt2, "unit": "clips/s", "ms_per_step": dt2 / args.steps * 1e3,
                   "steps": args.steps, "warmup": args.warmup, "dtype": DTYPES[other], "precision": other,
                   "stage_ms": dict((k, v[0] / max(v[1], 1)) for k, v in st2.items())}
            ip2 = roofline_in_path(_h2, _h2._feat_array(feats), out, B, L, other, min(args.steps, 20))
            sec["units_kernel"] = next((k for k in ip2["kernels"] if k["launch"].startswith("units:pw_tdiff")), None)
            sec["roofline_in_path"] = ip2
            del _h2
            ip_split, ip_f32 = (ip2, in_path) if other == "f32split" else (in_path, ip2)
            if ip_split is not None and ip_f32 is not None:
                # every launch that runs in split-fp32 arithmetic in that mode (the units kernel, the batched GEMMs of every conv on a
                # Winograd path, the 1x1 convs on 7x7 maps, the bottleneck chains), with the same launch's time in the fp32 mode beside it
                fp32_ms = dict((k["launch"], k["avg_ms"]) for k in ip_f32["kernels"])
                rows_ = []
                for k in ip_split["kernels"]:
                    nm = k["launch"]
                    if "flops" not in k or abs(k["avg_ms"] - fp32_ms.get(nm, k["avg_ms"])) < 0.02 * k["avg_ms"] and not nm.startswith("units:pw_tdiff"):
                        continue
                    if not (nm.startswith("units:pw_tdiff") or "GEMMs]" in nm or nm.startswith("chain_") or "between]" in nm or nm in SPLIT_1X1_LAUNCHES):
                        continue
                    rows_.append({"launch": nm, "avg_ms": k["avg_ms"], "fp32_mode_avg_ms": fp32_ms.get(nm), "flops_fp32_equivalent": k["flops"],
                                  "fp32_equivalent_tflops": k["flops"] / k["avg_ms"] / 1e9,
                                  "frac_of_bf16_peak": 6.0 * k.get("executed_flops", k["flops"]) / k["avg_ms"] / 1e9 / BF16_DENSE_PEAK_TFLOPS,
                                  "fp32_equivalent_over_fp32_pipe_peak": k["flops"] / k["avg_ms"] / 1e9 / MFMA_F32_PEAK_TFLOPS})
                res["split_launches"] = {"kernels": rows_, "sum_ms": sum(r["avg_ms"] for r in rows_),
                                         "sum_ms_fp32_mode": sum(r["fp32_mode_avg_ms"] or 0.0 for r in rows_),
                                         "note": "frac_of_bf16_peak = six bf16 plane products per fp32 product / 2.5 PF dense bf16; "
                                                 "everything else in the forward (transforms, heads) is the same code in both modes"}
            res["error_vs_fp64"] = split_error_vs_fp64(L, variant, weights, dev)
            res["gemm_error_vs_fp64"] = split_gemm_error_vs_fp64(dev)
            res["max_rel_diff_between_modes"] = split_vs_fp32_forward(B, L, variant, weights, dev)
            res["error_note"] = ("error_vs_fp64 / gemm_error_vs_fp64: the units kernel / the batched GEMMs of a Winograd conv in BOTH modes against an fp64 contraction of "
                                 "the same fp32 inputs -- the split mode's error is the smaller one on every input kind (asserted in "
                                 "tests/test_gpu_split.py): the operands are represented exactly, the products are exact, the running sum is "
                                 "rounded once per 32 k where the fp32 pipe's FMA chain rounds it eight times.  max_rel_diff_between_modes: "
                                 "the whole forward, one mode against the other (budget 1e-3)")
            res[("fp32_pipe" if other == "fp32" else other) + "_mode"] = sec
            # BASELINE config 3 (Flow_OFF, B = 64, fixed diagonal Sobel + SegmentConsensus) and config 5's per-GPU leg (RGB + Flow
            # on the same clips, two HIP streams, K7 late fusion incl. both TSN scores), in the headline's arithmetic
            res["flow_variant"] = flow_variant(B, L, dev, args.steps, args.warmup, measure, args.precision)
            res["two_stream"] = two_stream_leg(B, L, dev, args.steps, args.warmup, feats, weights, args.precision)
            res["units_training"] = [units_training(B, L, variant, weights, feats, dev, "fp32")]
            if not coll:
                res["rccl_single_rank_smoke"] = rccl_smoke_object(B, L, variant, weights, feats, dev, min(args.steps, 20), args.precision,
                                                                  args.collective)
            if args.cpu_clips > 0:
                res["cpu_baseline"] = cpu_baseline(feats_np, weights, L, variant, min(args.cpu_clips, B))
                res["gpu_over_cpu"] = clips_s / res["cpu_baseline"]["value"]
        emit(res, args.detail)
    if coll:
        dist.barrier()
    if dist.is_initialized():
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
