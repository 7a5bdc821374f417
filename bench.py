#!/usr/bin/env python3
"""Headline benchmark: ISP + YOLOv3 forward images/sec @1280x720, batch 8 per GPU (BASELINE.json configs[1]).

One "step" = one batch through the whole hot path with inputs resident in HBM:
    5 RL steps of the ISP (64x64 pooling -> policy/parameter heads -> selected filter kernel), teacher-forced
    schedule S_mixed = [E, CCM, NLM, Shr, T] so the kernel work is deterministic,
    then the YOLOv3 forward (letterbox 720->736 fused into the stem, bf16 MFMA convs, eval decode).
N GPUs = N independent replicas (one process per GPU, no data-path collective): scaling "weak".

    python bench.py --gpus 1 --steps 20 --warmup 3
    python bench.py --gpus 1 --steps 20 --warmup 3 --full
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...

Prints ONE JSON line (rank 0). A plain run sets up, warms up, times the steps, writes --dump-outputs and prints the headline
keys only. --full adds everything else, each outside the timed region: `single_stream` and `device_selected_path` (the
same steps launched other ways), `roofline` (dominant kernel = the conv kernel with the largest total time, timed per launch
with HIP events on the launch stream, inside the network, beside the ISP stream; the next three in `other_kernels`), `isp`
(per-step ISP kernel times vs the HBM roof), `h2d` and the other BASELINE configs (run_extras), and `cpu_baseline` (the
reference's op chain restated on torch-CPU + plain torch-CPU detector on a bounded sample, host cores of this box; 1 warm-up
+ 3 repeats, min/median). --no-detail / --no-extras / --no-cpu-baseline leave parts of that out again.
"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

SCHEDULES = {"mixed": [0, 2, 4, 3, 5], "point": [0, 9, 2, 5, 1], "heavy": [4, 3]}
NAMES = ["E", "G", "CCM", "Shr", "NLM", "T", "Ct", "S+", "BW", "W"]
HBM_PEAK_GBS = 8000.0          # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy ceiling)
MFMA_BF16_PEAK_TFLOPS = 2500.0  # dense bf16 peak
TUNE_CACHE = os.path.join(ROOT, "adaptiveisp_amd", "yolo", "tuning", "mi355x.json")
CONV_KERNEL_NAMES = {2: "dma::k_conv_igemm_dma<128,128,2,2,2>", 5: "dma2::k_conv_igemm_dma32<128,128,2,2,2,0,64,1>",
                     22: "dma2::k_conv_igemm_dma32<128,64,4,1,4,0,32,1>", 26: "dma2::k_conv_igemm_dma32<128,256,2,4,3,0,32,4>",
                     27: "dma2::k_conv_igemm_dma32<256,128,4,2,3,0,32,4>", 40: "smallk::k_conv3x3_small<...>",
                     50: "pp::k_conv_pp<0, false>", 57: "pp::k_conv_chain", 58: "pp::k_conv_pp<0, true>", 59: "bnk::k_bneck<0>", 61: "bws::k_bneck_ws", 60: "pp128::k_conv_pp128<0, false>", 70: "k1::k_conv_k1", 80: "pq::k_conv_pq<0, 4>", 85: "pq::k_conv_pq<0, 2>", 90: "ws::k_conv_ws"}


_T0 = time.perf_counter()


def mark(what):
    """Progress on stderr (never on stdout: that is the ONE JSON line): which phase a slow or hung run is in."""
    if os.environ.get("RANK", "0") == "0":
        print(f"[bench +{time.perf_counter() - _T0:6.1f}s] {what}", file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--schedule", default="mixed", choices=sorted(SCHEDULES))
    ap.add_argument("--no-graph", action="store_true", help="launch eagerly instead of replaying a hipGraph")
    ap.add_argument("--no-pipeline", action="store_true", help="one stream: the detector of a batch starts only after "
                    "its own ISP episode (no overlap of consecutive batches)")
    ap.add_argument("--pipeline", default="streams", choices=["interleaved", "streams"], help="how consecutive batches "
                    "overlap: `streams` = the whole ISP episode of the next batch on a second stream (build_pipeline); `interleaved` "
                    "= its filters between the detector's layers on one stream, only its policy launches on a second "
                    "(build_interleaved; measured 0.12-0.15 ms per step SLOWER, tools/pipeline_points_ab.py)")
    ap.add_argument("--retune", action="store_true", help="re-measure the per-layer conv variants instead of loading "
                    "adaptiveisp_amd/yolo/tuning/*.json")
    ap.add_argument("--full", action="store_true", help="after the headline, also measure everything else the line can carry "
                    "(other launch forms, per-kernel roofline, ISP kernels, h2d, BASELINE configs 3, 4, 5, cpu_baseline: "
                    "~2 minutes, outside the timed region); a plain run prints the headline alone")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip cpu_baseline")
    ap.add_argument("--no-detail", action="store_true", help="with --full: skip the other launch forms, the per-kernel "
                    "roofline passes and the extras")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip h2d and the extra keys for BASELINE configs 3, "
                    "4, 5 (train_iteration, eval_config3, config5, batch16, raw: ~1 minute)")
    ap.add_argument("--cpu-probe", type=int, default=0, help=argparse.SUPPRESS)      # child of cpu_baseline (all-cores figure)
    ap.add_argument("--raw", action="store_true", help="start every step from a uint16 RGGB Bayer plane in HBM (adaisp_demosaic, "
                    "an extension: the reference's pipeline starts from RGB) instead of the fp32 RGB batch")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="after the timed steps, write what the timed path "
                    "computed in its last step as DIR/<name>.npy (float32; a fixed, seeded sample of every array, indices beside "
                    "it as <name>_index.npy, float64; at most 64 MB in all): for comparing two builds output for output")
    a = ap.parse_args()
    if a.steps < 1:
        ap.error("--steps must be at least 1")
    if not a.full:                                        # a plain run: nothing beyond the headline
        a.no_detail = a.no_extras = a.no_cpu_baseline = True
    return a


def build_workload(a, dev):
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.yolo import YoloEngine, yolov3
    torch.manual_seed(0)
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=dev).to(dev).eval()
    torch.manual_seed(1)
    det = yolov3().eval()
    engine = YoloEngine(det, a.batch, a.height, a.width, device=dev)
    # one writer: rank 0 measures (if it has to) and rewrites the table, the other ranks read it after the barrier
    rank, world = int(os.environ.get("RANK", "0")), int(os.environ.get("WORLD_SIZE", "1"))
    if world > 1:
        import torch.distributed as dist
        if rank == 0:
            engine.autotune(cache=TUNE_CACHE, retune=a.retune)
        dist.barrier()
        if rank != 0:
            engine.autotune(cache=TUNE_CACHE, write=False)
    else:
        engine.autotune(cache=TUNE_CACHE, retune=a.retune)
    g = torch.Generator(device="cpu").manual_seed(1234 + 1)
    x0 = (torch.rand(a.batch, 3, a.height, a.width, generator=g) ** 2.2 * 0.5).to(dev)
    raw = None
    if getattr(a, "raw", False):
        # the same scene as a 16-bit RGGB colour-filter-array plane: R at (even, even), G at (even, odd) / (odd, even), B at (odd, odd)
        from adaptiveisp_amd import _lib as isp_lib
        q = (x0 * 65535.0).round().clamp(0, 65535).to(torch.int32)
        plane = q[:, 1].clone()
        plane[:, 0::2, 0::2] = q[:, 0, 0::2, 0::2]
        plane[:, 1::2, 1::2] = q[:, 2, 1::2, 1::2]
        raw = plane.to(torch.uint16).contiguous()
        isp_lib.demosaic(raw, out=x0)                      # x0 is from now on what the demosaic writes at the top of every step
    z = torch.rand(a.batch, cfg.z_dim, generator=g).to(dev)
    s0 = torch.zeros(a.batch, cfg.num_state_dim, device=dev)
    sched = SCHEDULES[a.schedule]
    # device_ids: the step is still teacher-forced (same schedule, same kernels' work), but the filter launch is NOT told the op:
    # it reads the per-image op ids from the device as a policy-selected step does (adaisp_forward: one launch per kernel
    # family + the selective pooling launch) instead of adaisp_forward_uniform's single launch
    # BENCH_EXPERIMENT_NO_POLICY=1 (a MEASUREMENT aid, never the reported line — main() refuses to print a headline with it): the
    # policy's launches of a half-step run once and their plan is reused by every later step, i.e. the episode's filters run without
    # the 30 policy launches beside them: what the policy's latency chain costs the pipelined step
    mode = {"device_ids": False, "cache_plans": os.environ.get("BENCH_EXPERIMENT_NO_POLICY") == "1", "plans": {}}

    def isp_chain(out=None, start=0, stop=None, carry=None, with_carry=False, pooled_out=None):
        """The 5-step episode, or a slice of it in HALF-steps: half-step 2i is step i's policy on the 64x64 pooling of
        its input (Agent.plan_step), 2i+1 its filter on the full-resolution batch (Agent.apply_step), which ALSO writes
        the pooling of its result — the next step's policy input — in the same launch; only the episode's first image is
        pooled by a launch of its own. `carry` = (image, states, pending plan, pooled planes of the image) continues a
        slice. `out` / `pooled_out`: where the slice's last filter writes (the pipeline's hand-over / mid-episode
        buffers). Half-steps [0, 2*len(sched)) in order are exactly Agent.forward step by step."""
        stop = 2 * len(sched) if stop is None else stop
        if raw is not None and start == 0 and carry is None:
            isp_lib.demosaic(raw, out=x0)                  # --raw: the episode starts from the Bayer plane
        x, st, plan, pooled = carry if carry is not None else (x0, s0, None, None)
        last_apply = max((h for h in range(start, stop) if h & 1), default=-1)
        with torch.no_grad():
            for h in range(start, stop):
                if h & 1:
                    last = h == last_apply
                    if (h >> 1) + 1 < len(sched):          # a next step exists: its policy input comes out of this launch
                        pooled = pooled_out if (last and pooled_out is not None) else x0.new_empty((a.batch, 3, 64, 64))
                    else:
                        pooled = None
                    x = agent.apply_step(x, plan, out=out if last else None, pooled_next=pooled)
                    plan = None
                else:
                    if mode["cache_plans"] and h in mode["plans"]:
                        plan = mode["plans"][h]
                    else:
                        plan = agent.plan_step((x, z, st), 1.0, selected_filter_id=sched[h >> 1], pooled=pooled)
                        if mode["cache_plans"]:
                            mode["plans"][h] = plan
                    if mode["device_ids"]:
                        plan["host_op"] = None
                    st, pooled = plan["new_states"], None
        return (x, st, plan, pooled) if with_carry else x

    def step():
        x = isp_chain()
        step.isp_out = x                                   # under capture: the graph's own output tensor, rewritten by every replay
        with torch.no_grad():
            return engine(x)

    step.isp_chain = isp_chain
    step.sched = sched
    step.mode = mode
    return step, engine, agent, x0, sched


def build_pipeline(step, engine, x0, cut=None, gate=None, detector_eager=False, two_graphs=None):
    """Two-stage software pipeline over consecutive batches, captured as two hipGraphs (even / odd): one replay runs
    one ISP episode's worth of work (latency-bound: pooling, policy heads, one filter kernel per RL step) on one stream
    and the detector forward of batch i (MFMA-bound) on another. Every replay still does one whole ISP pass and one
    whole detector pass; the hand-over tensor is double-buffered. Returns (prime, run): `prime()` fills the pipeline
    (untimed), `run()` advances it by one step.

    cut (in half-steps, see isp_chain): the ISP stream runs half-steps cut.. of batch i+1 and then 0..cut-1 of batch
    i+2 — the episode is cut there, image / states / pending plan wait in a double-buffered mid-episode slot; the PHASE
    of the ISP work against the detector's layers is chosen, not its amount. gate: how many of the ISP stream's
    half-steps run before the detector stream is released (0: both start together).
    Default: the cut is in front of the NLM step and both streams start together. tools/pipeline_phase_ab.py, interleaved
    in one process at config 2 (ms per step): no cut 4.36; cut in front of the NLM step 4.32 (either side of its policy
    half); NLM alone first, detector released after it 4.365; two or three half-steps alone 4.44-4.46. The step is the
    sum of the CU time of detector, NLM and the pointwise kernels in every arrangement — running NLM alone buys nothing,
    so the two do not fragment each other's CUs either.

    detector_eager: the measuring form of the SAME arrangement — the graphs hold only the ISP stream's part and `run()`
    launches the detector eagerly on the second stream beside the graph replay, so that its launches can be bracketed by
    HIP events (event-record nodes inside a captured graph are not available on this ROCm: round 3).

    two_graphs (BENCH_PIPELINE_GRAPHS=2; not the default): the two stages as TWO one-stream hipGraphs per step, each launched on its
    own stream and held in lockstep by events recorded and waited for BETWEEN the launches, instead of one graph with the detector
    forked onto the second stream inside it. A fork / join inside a hipGraph costs ~0.3 ms of idle device per replay in isolation
    (tools/graph_launch_gap.py) — measured here it costs this step nothing: 4.394 (one graph) against 4.405 ms, five
    interleaved rounds, host work per step 0.23 against 0.08 ms (tools/pipeline_graphs_ab.py, profiles/round6_pipeline_graphs_ab.txt);
    in this file's own timed loop, fresh processes interleaved, the two-graph form is the SLOWER one (4.79 against 4.37 ms).
    Same launches, same buffers, same dependencies (every part of step i after every part of step i - 1). Needs gate = 0."""
    if two_graphs is None:
        two_graphs = os.environ.get("BENCH_PIPELINE_GRAPHS", "1") == "2"
    sched = step.sched
    nh = 2 * len(sched)
    if cut is None:
        cut = 2 * sched.index(4) if 4 in sched else 0               # 4 = NLM
    gate = 0 if gate is None else gate
    if not 0 <= cut < nh:
        raise ValueError(f"cut={cut} outside the {nh} half-steps of the episode")
    xbuf = [torch.empty_like(x0), torch.empty_like(x0)]
    mid = [None, None]                                    # per slot: image, states, op ids, packed parameter rows, host-known op, pooled planes
    side = torch.cuda.Stream()
    # both stages on ordinary-priority streams: a high-priority stream for the ISP chain was measured 26 % SLOWER
    # (1039 vs 1407 images/s) — its NLM workgroups then pre-empt the detector's at every CU hand-over
    hp = torch.cuda.Stream()

    def head(p):                                          # half-steps 0 .. cut-1 of a fresh batch -> mid-episode slot p
        if mid[p] is None:
            x, st, plan, pooled = step.isp_chain(stop=cut, with_carry=True)
            mid[p] = [torch.empty_like(x0) if cut > 1 else None, torch.empty_like(st),
                      torch.empty_like(plan["op_ids"]) if plan else None, torch.empty_like(plan["packed"]) if plan else None,
                      plan["host_op"] if plan else None, torch.empty_like(pooled) if pooled is not None else None]
        x, st, plan, pooled = step.isp_chain(out=mid[p][0], stop=cut, with_carry=True, pooled_out=mid[p][5])
        mid[p][1].copy_(st)
        if plan:
            mid[p][2].copy_(plan["op_ids"])
            mid[p][3].copy_(plan["packed"])

    def carry(p):
        img, st, ids, packed, host_op, pooled = mid[p]
        return (img if img is not None else x0, st,
                {"op_ids": ids, "packed": packed, "host_op": host_op} if ids is not None else None, pooled)

    if cut:                                               # slots exist before capture (their addresses are baked in)
        head(0); head(1)
        torch.cuda.synchronize()
    two_graphs = bool(two_graphs) and not gate and not detector_eager
    graphs = []
    for p in range(2):
        if two_graphs:
            gi, gd = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(gi, stream=hp):
                step.isp_chain(out=xbuf[p], start=cut, carry=carry(1 - p) if cut else None)   # rest of batch i+1 -> hand-over buffer
                if cut:
                    head(p)                              # first half-steps of batch i+2 -> mid-episode slot
            with torch.cuda.graph(gd, stream=side), torch.no_grad():
                engine(xbuf[1 - p])                      # detector of the batch the previous replay retouched
            graphs.append((gi, gd))
            continue
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=hp):
            cur = torch.cuda.current_stream()
            c = carry(1 - p) if cut else None
            if gate:                                     # the ISP stream's first half-steps run alone
                c = step.isp_chain(out=xbuf[p] if cut + gate >= nh else None, start=cut, stop=min(cut + gate, nh), carry=c,
                                   with_carry=True)
            if not detector_eager:
                side.wait_stream(cur)
                with torch.cuda.stream(side), torch.no_grad():
                    engine(xbuf[1 - p])                  # detector of the batch the previous replay retouched
            if cut + gate < nh:
                step.isp_chain(out=xbuf[p], start=cut + gate, carry=c)   # rest of batch i+1 -> hand-over buffer
            if cut:
                head(p)                                  # first half-steps of batch i+2 -> mid-episode slot
            if not detector_eager:
                cur.wait_stream(side)
        graphs.append(g)
    state = {"i": 0}
    done = [torch.cuda.Event(), torch.cuda.Event()] if two_graphs else None     # (ISP stream, detector stream) of the last step

    def prime():
        step.isp_chain(out=xbuf[1])
        if cut:
            head(1)
        state["i"] = 0

    def run():
        p = state["i"] & 1
        if two_graphs:
            cur = torch.cuda.current_stream()
            for st in (hp, side):                        # what the caller enqueued (prime(), the previous step's consumers) first;
                st.wait_stream(cur)                      # both parts of step i after both parts of step i - 1
                if state["i"]:
                    st.wait_event(done[0])
                    st.wait_event(done[1])
            with torch.cuda.stream(hp):
                graphs[p][0].replay()
                done[0].record(hp)
            with torch.cuda.stream(side):
                graphs[p][1].replay()
                done[1].record(side)
            cur.wait_event(done[0])                      # the caller's stream sees the step as one unit, as with the one-graph form
            cur.wait_event(done[1])
            state["i"] += 1
            return
        if detector_eager:
            cur = torch.cuda.current_stream()
            side.wait_stream(cur)
            graphs[p].replay()                           # the ISP stream's part of this step ...
            with torch.cuda.stream(side), torch.no_grad():
                engine(xbuf[1 - p])                      # ... beside the detector, launch by launch
            cur.wait_stream(side)
        else:
            graphs[p].replay()
        state["i"] += 1

    run.xbuf, run.state = xbuf, state                    # (for the race screens: replay k leaves its episode in xbuf[k & 1])
    return prime, run


def build_interleaved(step, engine, x0, points=None, eager=False, side_priority=0):
    """The same software pipeline over consecutive batches — one replay = the ISP episode of batch i+1 and the detector
    forward of batch i — with the FILTER launches of the episode placed BETWEEN the detector's layers on the detector's own
    stream (YoloEngine.hook) and only the policy launches (six small latency-bound kernels per RL step) on a second stream.
    The idea: two streams share CUs by time-slicing whole workgroups, so every conv launch that overlaps an NLM or pointwise
    launch loses its CUs for that long (the fused pair: 115 us beside the ISP stream, 93 us alone); in series the conv kernels
    run at their clean time while the policy's latency chain stays hidden. MEASURED (round 4, tools/pipeline_points_ab.py, one
    process, 8x720x1280): the conv kernels do run at their clean time, but the step is 4.45-4.55 ms against 4.33 for the
    two-stream arrangement — the policy's six dependent small launches get CUs only at the conv launches' tails, so the
    filter that waits for them stalls the detector's stream, and the two-stream form overlaps some of NLM's VALU work with
    the conv kernels' memory phases. Not the default; kept as `--pipeline interleaved`. `points[k]` = detector launch index after which filter k is issued (default:
    spread over the first ~60 % of the forward so the chain pol -> filter -> pol ... always has a policy's worth of layers
    between two filters). Every replay still does one whole ISP pass and one whole detector pass. eager=True: the same
    schedule launched without a graph (the per-kernel event-pair timing uses it)."""
    sched = step.sched
    n = len(sched)
    L = engine.num_launches()
    if points is None:
        first, last = max(2, L // 12), max(n + 2, int(L * 0.62))
        points = [first + (last - first) * k // max(1, n - 1) for k in range(n)]
    if len(points) != n or any(b <= a for a, b in zip(points, points[1:])) or points[-1] >= L:
        raise ValueError(f"points {points}: need {n} increasing detector launch indices < {L}")
    at = {pt: k for k, pt in enumerate(points)}
    xbuf = [torch.empty_like(x0), torch.empty_like(x0)]
    side, hp = torch.cuda.Stream(priority=side_priority), torch.cuda.Stream()

    def body(p):
        cur = torch.cuda.current_stream()
        carry = [None]

        def half(h, out=None):
            carry[0] = step.isp_chain(out=out, start=h, stop=h + 1, carry=carry[0], with_carry=True)

        def hook(i):
            k = at.get(i)
            if k is None:
                return
            cur.wait_stream(side)                          # policy of RL step k has produced op ids / parameters
            half(2 * k + 1, out=xbuf[p] if k == n - 1 else None)      # filter k (+ the pooling of its result), in series
            if k + 1 < n:
                side.wait_stream(cur)
                with torch.cuda.stream(side):
                    half(2 * k + 2)                        # policy of step k + 1 beside the next layers
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            half(0)                                        # first input's pooling + policy of step 0
        done = [0]
        engine.hook = lambda i: (hook(i), done.__setitem__(0, done[0] + (i in at)))
        try:
            with torch.no_grad():
                engine(xbuf[1 - p])                        # detector of the batch the previous replay retouched
        finally:
            engine.hook = None
        cur.wait_stream(side)
        if done[0] != n:
            raise RuntimeError(f"interleaved pipeline: only {done[0]} of {n} filters were placed (this engine's forward "
                               "does not call the layer hook)")

    graphs = []
    if not eager:
        for p in range(2):
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=hp):
                body(p)
            graphs.append(g)
    state = {"i": 0}

    def prime():
        step.isp_chain(out=xbuf[1])
        state["i"] = 0

    def run():
        p = state["i"] & 1
        if eager:
            body(p)
        else:
            graphs[p].replay()
        state["i"] += 1

    run.xbuf, run.state, run.points = xbuf, state, points
    return prime, run


def time_isp_kernels(x0, sched, iters=24):
    """Per-op ISP kernel time (HIP events on the launch stream), algorithmic 24 B/px. Two figures per op:
      ms / GBps / frac_hbm   on a ROTATING set of NSETS input / output buffer pairs (12 x 88.5 MB = 1.06 GB at config 2, four
                             times the 256 MB Infinity Cache; rounds 1-3 rotated over 531 MB, which still flattered plain
                             loads by 10-25 %: tools/stream_ceiling.hip): every launch reads lines that have left the cache;
      warm_ms / warm_GBps    the same launch repeated on ONE pair (what rounds 1-2 reported): part of its traffic is
                             Infinity-Cache resident when the tensors fit."""
    from adaptiveisp_amd import _lib
    B, _, H, W = x0.shape
    npar = {0: 1, 1: 1, 2: 9, 3: 1, 4: 1, 5: 8, 6: 1, 7: 1, 8: 1, 9: 3}
    NSETS = max(3, min(6, int(1.1e9 // (2 * x0.numel() * 4)) + 1))      # >= 1 GB per cycle where the tensors allow it
    ins = [x0] + [x0.clone() for _ in range(NSETS - 1)]
    outs = [torch.empty_like(x0) for _ in range(NSETS)]
    res = {"rotation_MB": round(NSETS * 2 * x0.numel() * 4 / 1e6)}

    def graph_timed(launch, n, rotate=True):
        """ms per launch of `launch(k)` (k = buffer set), n launches captured in ONE hipGraph and replayed: the launches are
        30-40 us kernels, and the Python binding's per-call host work (argument checks, version bumps) is of that order —
        back-to-back eager calls measure the host, not the kernel (round 4: `with_pool_ms` read 38.6 us where the same
        launches through bare ctypes calls took 35-36, tools/isp_step_ab.py)."""
        for k in range(NSETS):
            launch(k)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for i in range(n):
                launch(i % NSETS if rotate else 0)
        g.replay()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay(); g.replay()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / (2 * n)

    def timed(op, p, n, rotate):
        return graph_timed(lambda k: _lib.process(op, ins[k], p, clip=True, out=outs[k]), n, rotate)

    pools = [torch.empty((B, 3, 64, 64), dtype=torch.float32, device=x0.device) for _ in range(NSETS)]

    def timed_step(op, p, n):
        """The RL step's form of the launch: host-known op + the next step's 64x64 pooling out of the same launch."""
        return graph_timed(lambda k: _lib.forward(ins[k], None, p, clip=True, out=outs[k], pooled=pools[k], host_op=op), n)

    pooled_out = [None] * NSETS

    def pool_launch(k):
        pooled_out[k] = _lib.pool64(ins[k])
    res["pool64"] = {"ms": round(graph_timed(pool_launch, iters), 4), "bytes_per_px": 12}
    for op in sorted(set(sched)):
        p = torch.rand(B, npar[op], device=x0.device) * 0.8 + 0.6
        n = 6 if op == 4 else iters
        ms, warm = timed(op, p, n, True), timed(op, p, n, False)
        gbs = 24.0 * B * H * W / (ms * 1e-3) / 1e9
        res[NAMES[op]] = {"ms": round(ms, 4), "GBps": round(gbs, 1), "frac_hbm": round(gbs / HBM_PEAK_GBS, 3),
                          "warm_ms": round(warm, 4), "warm_GBps": round(24.0 * B * H * W / (warm * 1e-3) / 1e9, 1),
                          # the launch as the RL step issues it: + the next step's pooled planes (fused; NLM: + a pooling launch)
                          "with_pool_ms": round(timed_step(op, torch.nn.functional.pad(p, (0, 24 - p.shape[1])), n), 4)}
        if op == 4:        # NLM is bound by the fp32 VALU, not HBM: 4.6 kflop/px in the reference's arithmetic
            tf = 4.6e3 * B * H * W / (ms * 1e-3) / 1e12
            res[NAMES[op]].update({"bound": "fp32 valu", "ref_arith_TFLOPs": round(tf, 1), "peak_TFLOPs": 157.3,
                                   "frac_valu": round(tf / 157.3, 3)})
    return res


def time_conv_kernels(engine, x, reps=20, runner=None):
    """Per-launch duration of EVERY conv kernel of the detector, measured IN the network, twice:
      clean      the detector alone on its stream, `reps` forwards — kernel quality;
      pipelined  the arrangement the headline is timed in (`runner` = build_pipeline(..., detector_eager=True): the ISP
                 stream's part of the step replayed as a hipGraph beside the eagerly launched detector) — the detector's
                 workgroups share the CUs with NLM's there, which is what rocprofv3 --kernel-trace --stats of the same
                 command sees (profiles/).
    Every conv launch is bracketed by a HIP event pair on the stream it is launched on. Launch counts come from the PLAN (the
    launches `engine.forward` actually issues: the two head convs that live inside k_stem_down are not plan launches), the
    event list only supplies durations. Returns per kernel: launches per forward, both averages, flops per launch, TFLOP/s of
    both, share of the summed conv time; the DOMINANT kernel is the one with the largest total pipelined TIME."""
    FUSED = 58                     # pseudo-variant: variant 50 with the next block's 1x1 fused into its epilogue

    def entry(kind, args):
        """(variant, flops) of a conv launch of the plan; (None, 0) for everything else."""
        if kind == "bneck":             # a whole Bottleneck of the C = 256 stage: 1x1 256 -> 128 and 3x3 128 -> 256
            B, H, W = args[8:11]
            return 59, 2.0 * B * H * W * (256 * 128 + 9 * 128 * 256)
        if kind == "chain":             # a run of 256 x 256-kernel layers as one persistent launch (YoloEngine.fuse_chains)
            return 57, next(c["flops"] for c in engine.chains if c["ws"].data_ptr() == args[2].value)
        if kind == "bneckws":           # a whole Bottleneck of the C = 64 / 128 stages (YoloEngine.fuse_bottlenecks_ws)
            B, H, W, C = args[8:12]
            return 61, 2.0 * B * H * W * (C * (C // 2) + 9 * (C // 2) * C)
        if kind == "k1":                # a 1x1 layer on the whole-K kernel (YoloEngine.fuse_k1)
            B, H, W, cin, cout = args[6:11]
            return 70, 2.0 * B * H * W * cin * cout
        if kind not in ("conv", "conv2"):
            return None, 0.0
        B, H, W, cin, cout, k, s = args[8:15]
        Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
        fl = 2.0 * B * Ho * Wo * cout * k * k * cin
        if kind == "conv2":
            return FUSED, fl + 2.0 * B * Ho * Wo * cout * args[20]
        return args[16], fl

    pairs = []

    def bracket(fn, variant, flops):
        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = fn(*a)
            e1.record()
            pairs.append((e0, e1, variant, flops))
            return rc
        return call

    plan, wrapped, per_fwd, fl_fwd = engine.plan, [], {}, {}
    # the head of the plan that engine.forward does NOT launch from the plan (stem, and the convs fused into k_stem_down)
    skip = 0
    if getattr(engine, "_stem", None) is not None:
        skip = (3 if engine._head_next is not None else 2) if engine.fuse_head else 1
    for i, (kind, fn, args) in enumerate(plan):
        v, fl = entry(kind, args)
        if v is not None and i >= skip:
            wrapped.append((kind, bracket(fn, v, fl), args))
            per_fwd[v] = per_fwd.get(v, 0) + 1
            fl_fwd[v] = fl_fwd.get(v, 0.0) + fl
        else:
            wrapped.append((kind, fn, args))

    def measure(call):
        del pairs[:]
        engine.plan = wrapped
        try:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        finally:
            engine.plan = plan
        ms, n = {}, {}
        for e0, e1, v, fl in pairs:
            ms[v] = ms.get(v, 0.0) + e0.elapsed_time(e1)
            n[v] = n.get(v, 0) + 1
        bad = {v: n.get(v, 0) for v in per_fwd if n.get(v, 0) != per_fwd[v] * reps}
        if bad:
            raise RuntimeError(f"per-kernel timing: event pairs per variant {bad} do not match plan launches x reps")
        return {v: ms[v] / n[v] for v in ms}

    engine(x)
    torch.cuda.synchronize()
    clean = measure(lambda: engine(x))
    piped = measure(runner) if runner is not None else dict(clean)
    total = sum(piped[v] * per_fwd[v] for v in piped)
    table = []
    for v in per_fwd:
        fl = fl_fwd[v] / per_fwd[v]
        table.append({"variant": v, "kernel": CONV_KERNEL_NAMES.get(v, f"conv variant {v}"), "launches_per_step": per_fwd[v],
                      "avg_launch_ms": piped[v], "avg_launch_ms_clean": clean[v], "flops_per_launch": fl,
                      "tflops": fl / (piped[v] * 1e-3) / 1e12, "tflops_clean": fl / (clean[v] * 1e-3) / 1e12,
                      "share_of_conv_time": piped[v] * per_fwd[v] / total})
    table.sort(key=lambda r: -r["share_of_conv_time"])
    # whole detector forward alone on its stream, for the end-to-end TFLOP/s
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        engine(x)
    e1.record()
    torch.cuda.synchronize()
    det_ms = e0.elapsed_time(e1) / reps
    return {"kernels": table, "detector_ms": det_ms, "detector_tflops": engine.flops / (det_ms * 1e-3) / 1e12, "reps": reps}


def newest_profiles(suffix):
    """profiles/roundN_<suffix> of the NEWEST round any file under profiles/ belongs to — never an older round's file: a
    number taken from a profile two rounds old is not evidence for this tree. [] if that round has none."""
    import glob
    import re
    rounds = [int(m.group(1)) for m in (re.match(r"round(\d+)_", os.path.basename(f))
                                        for f in glob.glob(os.path.join(ROOT, "profiles", "round*_*"))) if m]
    if not rounds:
        return []
    return sorted(glob.glob(os.path.join(ROOT, "profiles", f"round{max(rounds)}_*{suffix}")), reverse=True)


def pmc_traffic(kernel_name):
    """HBM bytes per launch of `kernel_name` from the newest committed PMC passes (profiles/*_pmc_traffic.json, produced
    by tools/refresh_profiles.sh: separate --pmc runs, FETCH_SIZE x2 per the gfx950 note), averaged over the launches
    of that kernel in the benchmarked network (records are per launch geometry). None if not collected."""
    import glob
    key = kernel_name.split("::")[-1].replace(" ", "")
    if not key:
        return None, None
    for path in newest_profiles("pmc_traffic.json"):
        try:
            table = json.load(open(path))
        except Exception:
            continue
        recs = table if isinstance(table, list) else [dict(kernel=k, **v) for k, v in table.items()]
        hit = [r for r in recs if key in r["kernel"].replace(" ", "")]
        n = sum(r["launches"] for r in hit)
        if n:
            return sum(r["hbm_bytes_per_launch"] * r["launches"] for r in hit) / n, os.path.relpath(path, ROOT)
    return None, None


def rocprof_reference(kernel_name):
    """(average launch ms, file) of `kernel_name` in the newest committed rocprofv3 --kernel-trace --stats summary of this
    bench (profiles/*_rocprofv3_kernel_stats.csv) — printed beside the live figure; (None, None) if absent."""
    import csv
    import glob
    key = kernel_name.split("::")[-1].replace(" ", "")
    for path in newest_profiles("rocprofv3_kernel_stats.csv"):
        try:
            for r in csv.DictReader(open(path)):
                if key and key in r["Name"].replace(" ", ""):
                    return float(r["AverageNs"]) * 1e-6, os.path.relpath(path, ROOT)
        except Exception:
            continue
    return None, None


def rocprof_top_conv_kernel(kernels):
    """The entry of `kernels` (time_conv_kernels' table) whose kernel is the highest row of the newest committed rocprofv3
    kernel-stats CSV that names one of them; None without a profile."""
    import csv
    names = {r["kernel"].split("::")[-1].replace(" ", ""): r for r in kernels}
    for path in newest_profiles("rocprofv3_kernel_stats.csv"):
        try:
            rows = sorted(csv.DictReader(open(path)), key=lambda r: -float(r["TotalDurationNs"]))
        except Exception:
            continue
        for r in rows:
            nm = r["Name"].replace(" ", "")
            for key, ent in names.items():
                if key and key in nm:
                    return ent
    return None


def _timed(fn, repeats=3):
    """1 warm-up + `repeats` timed runs -> (min, median) seconds (SURVEY 8(d) protocol)."""
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[0], ts[len(ts) // 2]


ALL_CORES_LIMIT_S = 60


def cpu_probe(a, threads):
    """Child of cpu_baseline: the reference-faithful ISP step and the fp32 detector on ONE image with `threads` torch threads,
    1 warm-up + 1 repeat each -> one JSON line. No GPU is touched."""
    import numpy as np
    from oracle import torch_ref
    from adaptiveisp_amd.yolo import yolov3
    torch.set_num_threads(threads)
    sched = SCHEDULES[a.schedule]
    rng = np.random.default_rng(1235)
    x = torch.from_numpy((rng.random((1, 3, a.height, a.width)) ** 2.2 * 0.5).astype(np.float32))
    params = [torch.from_numpy((rng.random((1, torch_ref.NUM_PARAMS[op])) * 0.8 + 0.6).astype(np.float32)) for op in range(10)]
    params[4] = torch.full((1, 1), 0.2)
    sel = torch.tensor([sched[2 % len(sched)]])
    torch.manual_seed(1)
    det = yolov3().eval()
    Hp = (a.height + 31) // 32 * 32
    boxed = torch.full((1, 3, Hp, a.width), 114 / 255)
    with torch.no_grad():
        sa, _ = _timed(lambda: torch_ref.policy_step(x, params, sel), repeats=1)
        da, _ = _timed(lambda: det(boxed), repeats=1)
    print(json.dumps({"threads": threads, "isp_step_s": sa, "detector_s": da}), flush=True)


def cpu_baseline(a, sched):
    """The hot path on the host cores of this box, on a BOUNDED sample: ONE image of the batch. Three ISP figures, each
    1 warm-up + 3 repeats (min / median):
      reference_faithful  oracle/torch_ref.py, the reference's own formulation: every RL step runs ALL 10 filters on the
                          image (roll-based NLM, 8-pass tone, masked HSV), stacks them and keeps one by one-hot
                          multiply-sum (agent.py:103-116,154); one step is timed, the episode is 5 of them (its cost
                          does not depend on which filter is selected);
      selected_only       the same torch ops, only the scheduled filter per step (5 steps timed);
      c_oracle            oracle/isp_oracle.c (per-pixel gather form, OpenMP), the parity checker, 5 steps timed.
    The detector is the plain fp32 module tree on torch-CPU with a warm-up. `value` = images/sec of
    reference_faithful ISP + detector (medians)."""
    import numpy as np
    import oracle
    from oracle import torch_ref
    from adaptiveisp_amd.yolo import yolov3
    oracle.build()
    ncpu = os.cpu_count() or 1
    threads = max(1, min(ncpu, 64))          # one socket's worth: more threads only add oneDNN/OpenMP hand-over cost
    torch.set_num_threads(threads)
    rng = np.random.default_rng(1235)
    x_np = (rng.random((1, 3, a.height, a.width)) ** 2.2 * 0.5).astype(np.float32)
    x = torch.from_numpy(x_np)
    ops = list(range(10))
    params = [torch.from_numpy((rng.random((1, torch_ref.NUM_PARAMS[op])) * 0.8 + 0.6).astype(np.float32)) for op in ops]
    params[4] = torch.full((1, 1), 0.2)      # NLM h
    with torch.no_grad():
        sel = torch.tensor([sched[2 % len(sched)]])
        step_min, step_med = _timed(lambda: torch_ref.policy_step(x, params, sel))

        def selected_chain():
            cur = x
            for op in sched:
                F.adaptive_avg_pool2d(cur, 64)
                cur = torch_ref.forward(op, cur, params[op])
            return cur
        import torch.nn.functional as F
        so_min, so_med = _timed(selected_chain)

    def c_chain():
        cur = x_np
        for op in sched:
            oracle.pool64(cur)
            cur = oracle.forward(cur, op, params[op].numpy(), clip=True)
        return cur
    c_min, c_med = _timed(c_chain)
    cur = c_chain()
    torch.manual_seed(1)
    det = yolov3().eval()
    Hp = (a.height + 31) // 32 * 32
    boxed = torch.full((1, 3, Hp, a.width), 114 / 255)
    boxed[:, :, (Hp - a.height) // 2:(Hp - a.height) // 2 + a.height] = torch.from_numpy(cur)
    with torch.no_grad():
        d_min, d_med = _timed(lambda: det(boxed))
    nsteps = len(sched)
    isp_ref = nsteps * step_med
    # ONE whole-batch pass (no repeats: ~10-20 s) beside the 1-image sample: checks, once per run, the assumption that the
    # batch costs `batch` x the sample (BASELINE.md 3 quotes the metric at batch 8)
    batch_check = None
    try:
        xb = torch.from_numpy((rng.random((a.batch, 3, a.height, a.width)) ** 2.2 * 0.5).astype(np.float32))
        pb = [p.expand(a.batch, -1).contiguous() for p in params]
        with torch.no_grad():
            t0 = time.perf_counter()
            torch_ref.policy_step(xb, pb, sel.expand(a.batch).contiguous())
            sb = time.perf_counter() - t0
            t0 = time.perf_counter()
            det(boxed.expand(a.batch, -1, -1, -1).contiguous())
            db = time.perf_counter() - t0
        vb = a.batch / (nsteps * sb + db)
        batch_check = {"batch": a.batch, "isp_step_s": round(sb, 3), "detector_s": round(db, 3), "images_per_sec": round(vb, 4),
                       "vs_one_image_sample": round(vb / (1.0 / (isp_ref + d_med)), 3), "repeats": 1}
    except Exception as e:                                   # noqa: BLE001
        batch_check = {"error": f"{type(e).__name__}: {e}"}
    # BASELINE.md 3 says "all host cores": the same two timings once more with every hardware thread (1 warm-up + 1 repeat),
    # so that the 64-thread choice above is evidence in the line, not an assertion
    # (in a CHILD process with a time limit: with more OpenMP threads than the box's CPU quota allows, every parallel region of
    # the ~2000-op reference step degenerates into spin-waits — the probe then reports the limit instead of stalling the bench)
    all_cores = None
    if ncpu > threads:
        import subprocess
        # every hardware thread first; if that does not finish inside its limit (on this pool's hosts the 256-thread run of the
        # ~2000-op reference step degenerates into OpenMP spin-waits), half of them — so that `all_cores` carries a NUMBER
        # (VERDICT r5 item 7), plus the record of what timed out
        tried = []
        # (every hardware thread gets half the limit: on this pool it has never finished — rounds 5 and 6 — and the line should not
        # spend a minute finding that out again; half of them get the full limit)
        for nthr, limit in ((ncpu, ALL_CORES_LIMIT_S // 2), (max(threads + 1, ncpu // 2), ALL_CORES_LIMIT_S)):
            if nthr <= threads or any(t["threads"] == nthr for t in tried):
                continue
            mark(f"cpu_baseline: all-cores probe ({nthr} threads, child process, {limit} s limit)")
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-probe", str(nthr), "--height", str(a.height),
                                    "--width", str(a.width), "--schedule", a.schedule], capture_output=True, text=True,
                                   timeout=limit, cwd=ROOT)
                rec = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
                sa, da = rec["isp_step_s"], rec["detector_s"]
                all_cores = {"threads": nthr, "isp_step_s": round(sa, 3), "detector_s": round(da, 3),
                             "value": round(1.0 / (nsteps * sa + da), 4), "unit": "images/sec",
                             "images_per_sec": round(1.0 / (nsteps * sa + da), 4), "repeats": 1,
                             "vs_value": round((1.0 / (nsteps * sa + da)) / (1.0 / (isp_ref + d_med)), 3), "timed_out": tried}
                break
            except subprocess.TimeoutExpired:
                tried.append({"threads": nthr, "timeout_s": limit})
            except Exception as e:                               # noqa: BLE001
                tried.append({"threads": nthr, "error": f"{type(e).__name__}: {e}"})
        if all_cores is None:
            all_cores = {"timed_out": tried,
                         "note": f"1 warm-up + 1 repeat of the reference step and the detector did not finish within the limit at any "
                                 f"thread count above {threads} (the {threads}-thread figure takes ~{2 * (step_med + d_med):.0f} s for the same work)"}
    r3 = lambda v: round(v, 3)  # noqa: E731
    return {"all_cores": all_cores, "value": round(1.0 / (isp_ref + d_med), 4), "value_from": "medians", "value_min_times": round(1.0 / (nsteps * step_min + d_min), 4),
            "unit": "images/sec", "cores": threads, "kind": "port",
            "threads": threads, "threads_reason": f"min(os.cpu_count()={ncpu}, 64): one socket's worth — beyond it torch-CPU's oneDNN / "
                                                  "OpenMP hand-over cost grows faster than the work shrinks (BASELINE.md 3 asks for "
                                                  "all cores: `all_cores` holds the same timings with every hardware thread, "
                                                  "and the C oracle line below uses them all)",
            "sample": f"1 image of the batch @{a.width}x{a.height}; ISP = {nsteps} x one reference-faithful RL step (all 10 "
                      f"filters + one-hot select, torch-CPU op-for-op restatement oracle/torch_ref.py, median {step_med:.2f} s "
                      f"per step) + YOLOv3 fp32 torch-CPU forward (median {d_med:.2f} s); 1 warm-up + 3 repeats each; "
                      f"batch_check = one whole-batch pass of the same",
            "protocol": "1 warm-up + 3 repeats, min/median", "torch": torch.__version__, "host_cpus": ncpu,
            "isp_reference_faithful_s": {"per_step_min": r3(step_min), "per_step_median": r3(step_med),
                                         "episode_median": r3(isp_ref), "episode_min": r3(nsteps * step_min)},
            "isp_selected_only_s": {"schedule": [NAMES[k] for k in sched], "min": r3(so_min), "median": r3(so_med)},
            "isp_c_oracle_s": {"schedule": [NAMES[k] for k in sched], "min": r3(c_min), "median": r3(c_med),
                               "threads": ncpu},
            "detector_s": {"min": r3(d_min), "median": r3(d_med)}, "batch_check": batch_check}


def extra_train_iteration(dev, iters=8):
    """BASELINE config 4, one rank's share (batch 8 x 512 x 512; train.py:234-351): ms per RL iteration on the HIP training
    engine, the host's enqueue work and its waits for the GPU (what tools/train_bench.py prints), and the summed kernel time
    of two iterations under torch.profiler (None if the profiler is unavailable)."""
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.train import build_trainer
    from adaptiveisp_amd import train as atrain
    tr = build_trainer(cfg, 0, 1, dev, 8, 512, tune_cache=TUNE_CACHE)
    tr.train(tr.graph_warmup + 3 if tr.graph_mode else 3)    # (graph mode: the ordinary iterations, the capture, two replays)
    torch.cuda.synchronize()
    waited = [0.0]
    ev_sync, to_cpu, wait_guard = torch.cuda.Event.synchronize, torch.Tensor.cpu, atrain._GraphIteration.wait_guard

    def timed(fn):
        def call(*x, **k):
            t = time.perf_counter()
            r = fn(*x, **k)
            waited[0] += time.perf_counter() - t
            return r
        return call
    torch.cuda.Event.synchronize, torch.Tensor.cpu = timed(ev_sync), timed(to_cpu)     # the host's waits for the GPU
    atrain._GraphIteration.wait_guard = timed(wait_guard)    # (graph mode: the poll for the guard's flag, ~1 ms into the iteration)
    try:
        t0 = time.perf_counter()
        for _ in range(iters):
            tr.step()
        t_host = time.perf_counter() - t0
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / iters
    finally:
        torch.cuda.Event.synchronize, torch.Tensor.cpu = ev_sync, to_cpu
        atrain._GraphIteration.wait_guard = wait_guard
    kernel_ms = n_kernels = None
    try:
        if tr.graph_mode:                                    # (the profiler sees only part of a replayed graph's kernels: no figure
            raise RuntimeError("graph mode")                 #  rather than a wrong one; tools/train_timeline.sh traces the loop)
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(2):
                tr.step()
            torch.cuda.synchronize()
        evs = [e for e in prof.events() if e.device_type is not None and "cuda" in str(e.device_type).lower()]
        kernel_ms = sum(e.device_time for e in evs) / 2 / 1e3
        n_kernels = len(evs) // 2
    except Exception as e:                                   # noqa: BLE001 (measurement aid only)
        if str(e) != "graph mode":
            print(f"[bench] train_iteration: kernel time unavailable ({type(e).__name__}: {e})", file=sys.stderr)
    tr.materialize()
    return {"workload": "config 4, per rank: RL iteration (agent + value + replay + frozen YOLOv3 on the input and the retouched batch + data gradient) batch 8 x 512x512",
            "detector": "one 16-image forward + 8-image backward" if hasattr(tr.detector, "half") else "two 8-image forwards + backward",
            "one_hipgraph_per_iteration": bool(tr.graph_mode and tr._git is not None and tr._git.graph is not None),
            "ms_per_iteration": round(dt * 1e3, 2), "images_per_sec": round(8 / dt, 1), "iters": iters,
            "host_enqueue_ms": round((t_host - waited[0]) / iters * 1e3, 2), "host_wait_ms": round(waited[0] / iters * 1e3, 2),
            "kernel_ms": round(kernel_ms, 2) if kernel_ms is not None else None, "kernels_per_iteration": n_kernels}


def extra_eval_config3(dev, images=24):
    """BASELINE config 3's loop at its shape (val_adaptiveisp.py:287-310: batch 1, 512 x 512 letterbox, 5 ISP steps with the
    per-step early-exit check, detector, NMS at conf 0.001, matching) on synthetic frames + labels, random-init weights:
    the mAP means nothing, the time per image does."""
    from adaptiveisp_amd.agent import Agent
    from adaptiveisp_amd.config import cfg
    from adaptiveisp_amd.val.harness import run_eval
    from adaptiveisp_amd.yolo import YoloEngine, yolov3
    torch.manual_seed(0)
    agent = Agent(cfg, shape=(6 + len(cfg.filters), 64, 64), device=dev).to(dev).eval()
    torch.manual_seed(1)
    eng = YoloEngine(yolov3().eval(), 1, 512, 512, device=dev)
    eng.autotune(cache=TUNE_CACHE)
    g = torch.Generator().manual_seed(1)

    def batches(k):
        out = []
        for i in range(k):
            im = torch.rand(1, 3, 512, 512, generator=g) ** 2.2 * 0.5
            t = torch.zeros(3, 6)
            t[:, 1] = torch.randint(0, 80, (3,), generator=g).float()
            t[:, 2:4] = torch.rand(3, 2, generator=g) * 0.6 + 0.2
            t[:, 4:6] = torch.rand(3, 2, generator=g) * 0.3 + 0.05
            out.append((im.pin_memory(), t, [f"img{i}.png"], [((512, 512), ((1.0, 1.0), (0.0, 0.0)))]))
        return out
    data = batches(images)
    out = {}
    for key, graph in (("eager", False), ("graph", True)):  # the reference's loop launch by launch / one hipGraph replay per image
        run_eval(agent, eng, data[:3], cfg, graph=graph)     # warm-up (and, with graph=True, a throw-away capture)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = run_eval(agent, eng, data, cfg, graph=graph)
        torch.cuda.synchronize()
        out[key] = (time.perf_counter() - t0, int(res["seen"]))
    dt, seen = out["eager"]
    dtg = out["graph"][0]
    return {"workload": "config 3 loop: batch 1 x 512x512, 5 ISP steps (early-exit check) + YOLOv3 + NMS + matching, synthetic frames",
            "ms_per_image": round(dt / images * 1e3, 2), "images_per_sec": round(images / dt, 1), "images": images, "seen": seen,
            # run_eval(graph=True): episode + detector of an image as ONE hipGraph replay (the capture itself is inside this time:
            # one per run_eval call) — same records / detections / mAP (tests/test_gpu_eval.py)
            "graph_ms_per_image": round(dtg / images * 1e3, 2), "graph_images_per_sec": round(images / dtg, 1)}


def extra_config5(dev, steps=6):
    """BASELINE config 5: 4 x 3840x2160, denoise + sharpen (S_heavy) + YOLOv3 forward @3840x2176, same pipelined harness."""
    import types
    a5 = types.SimpleNamespace(batch=4, height=2160, width=3840, schedule="heavy", no_graph=False, no_pipeline=False,
                               retune=False, raw=False)
    run, single_run, graphed, pipelined, engine, x0, sched, step = prepare_gpu_run(a5, dev)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    k = time_isp_kernels(x0, sched, iters=6)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        engine(x0)
        e0.record()
        for _ in range(3):
            engine(x0)
        e1.record()
    torch.cuda.synchronize()
    det_ms = e0.elapsed_time(e1) / 3
    return {"workload": "config 5: batch 4 x 3840x2160, schedule [NLM, Shr] + YOLOv3 forward @3840x2176 bf16",
            "images_per_sec": round(4 / dt, 1), "ms_per_step": round(dt * 1e3, 2), "steps": steps,
            "launch_mode": (pipelined if pipelined == "interleaved" else "pipelined") if pipelined else ("graph" if graphed else "eager"),
            "nlm_ms": k["NLM"]["ms"], "nlm_frac_valu": k["NLM"].get("frac_valu"), "sharpen_ms": k["Shr"]["ms"],
            "sharpen_frac_hbm": k["Shr"]["frac_hbm"], "sharpen_with_pool_ms": k["Shr"]["with_pool_ms"],
            "detector_ms": round(det_ms, 3), "detector_tflops": round(engine.flops / (det_ms * 1e-3) / 1e12, 1)}


def extra_batch16(dev, steps=12):
    """The headline's workload at TWICE the batch (16 x 1280x720, same schedule, same pipelined harness): what the detector's
    deep layers — 23 x 40 maps, 116-232 tiles for 256 CUs at batch 8 — leave on the table at the named batch size. Not the
    headline: BASELINE's config is batch 8."""
    import types
    a16 = types.SimpleNamespace(batch=16, height=720, width=1280, schedule="mixed", no_graph=False, no_pipeline=False,
                                retune=False, raw=False)
    run, single_run, graphed, pipelined, engine, x0, sched, step = prepare_gpu_run(a16, dev)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.no_grad():
        engine(x0)
        e0.record()
        for _ in range(5):
            engine(x0)
        e1.record()
    torch.cuda.synchronize()
    det_ms = e0.elapsed_time(e1) / 5
    return {"workload": "the headline's step at batch 16 x 1280x720 (NOT the BASELINE config: batch 8)", "images_per_sec": round(16 / dt, 1),
            "ms_per_step": round(dt * 1e3, 2), "steps": steps,
            "launch_mode": (pipelined if pipelined == "interleaved" else "pipelined") if pipelined else ("graph" if graphed else "eager"),
            "detector_ms": round(det_ms, 3), "detector_ms_per_image": round(det_ms / 16, 4),
            "detector_tflops": round(engine.flops / (det_ms * 1e-3) / 1e12, 1)}


def extra_raw(dev, steps=12):
    """The headline's step fed from a uint16 RGGB Bayer plane resident in HBM (adaisp_demosaic at the top of every episode, then
    the same 5 ISP steps + detector; `--raw` of the command line) — SURVEY 8(d)'s "Bayer input as a separate line". An
    extension: the reference's pipeline starts from RGB (yolov3/val_adaptiveisp.py:276-278; isp/unprocess_np.py:82-128 packs)."""
    import types
    ar = types.SimpleNamespace(batch=8, height=720, width=1280, schedule="mixed", no_graph=False, no_pipeline=False,
                               retune=False, raw=True)
    run, single_run, graphed, pipelined, engine, x0, sched, step = prepare_gpu_run(ar, dev)
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        run()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"workload": "batch 8 x 1280x720 uint16 RGGB Bayer plane (14.7 MB) -> demosaic -> the headline's 5-step ISP + YOLOv3 forward",
            "images_per_sec": round(8 / dt, 1), "ms_per_step": round(dt * 1e3, 3), "steps": steps,
            "launch_mode": (pipelined if pipelined == "interleaved" else "pipelined") if pipelined else ("graph" if graphed else "eager")}


def measure_h2d(a, dev, run, step_ms, reps=10, steps=12):
    """The feed, measured (outside the timed region): one batch from PINNED host memory to HBM on a copy stream — alone, and one
    copy per step beside the running headline pipeline — for the fp32 RGB batch the reference's loader hands over
    (yolov3/val_adaptiveisp.py:276-278: uint8 -> float / 255 on the device; the fp32 form is the upper bound) and for the
    uint16 Bayer plane of the `raw` line. HIP events on the copy stream; `step_ms_with_copy` is the wall time per step of
    the same pipeline while the copies run."""
    out = {"link": "PCIe Gen5 x16, 63 GB/s spec (MI355X_MICROARCH.md)", "pinned": True}
    copy = torch.cuda.Stream(device=dev)
    for name, shape, dtype in (("fp32_rgb", (a.batch, 3, a.height, a.width), torch.float32),
                               ("uint16_bayer", (a.batch, a.height, a.width), torch.uint16)):
        try:
            host = torch.zeros(shape, dtype=dtype).pin_memory()
            dst = torch.empty(shape, dtype=dtype, device=dev)
            nbytes = host.numel() * host.element_size()
            torch.cuda.synchronize()
            with torch.cuda.stream(copy):
                dst.copy_(host, non_blocking=True)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    dst.copy_(host, non_blocking=True)
                e1.record()
            copy.synchronize()
            alone = e0.elapsed_time(e1) / reps
            pairs = []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                with torch.cuda.stream(copy):
                    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    c0.record()
                    dst.copy_(host, non_blocking=True)
                    c1.record()
                pairs.append((c0, c1))
                run()
            torch.cuda.synchronize()
            with_copy = (time.perf_counter() - t0) / steps * 1e3
            beside = sum(c0.elapsed_time(c1) for c0, c1 in pairs) / len(pairs)
            out[name] = {"bytes": nbytes, "alone_ms": round(alone, 3), "alone_GBps": round(nbytes / alone / 1e6, 1),
                         "beside_a_step_ms": round(beside, 3), "beside_a_step_GBps": round(nbytes / beside / 1e6, 1),
                         "step_ms_with_copy": round(with_copy, 3), "step_ms_without": round(step_ms, 3)}
            del host, dst
        except Exception as e:                               # noqa: BLE001
            out[name] = {"error": f"{type(e).__name__}: {e}"}
    return out


def run_extras(dev, line):
    """Configs 3, 4, 5 as short extra keys of the driver's line — OUTSIDE the headline's timed region, each freed before the
    next; a failure is recorded in its key, never raised."""
    import gc
    for key, fn in (("train_iteration", extra_train_iteration), ("eval_config3", extra_eval_config3), ("config5", extra_config5),
                    ("batch16", extra_batch16), ("raw", extra_raw)):
        t0 = time.perf_counter()
        mark(f"extra: {key}")
        try:
            line[key] = fn(dev)
        except Exception as e:                               # noqa: BLE001
            line[key] = {"error": f"{type(e).__name__}: {e}"}
        line[key]["wall_s"] = round(time.perf_counter() - t0, 1)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


DUMP_SAMPLES = 1 << 21      # elements kept per array: 2 arrays x 2^21 x (4 B value + 8 B index) = 48 MB in all


def dump_outputs(outdir, arrays):
    """--dump-outputs: every array of `arrays` (name -> device tensor) as DIR/<name>.npy, float32. One of more than DUMP_SAMPLES
    elements is written as a sample: the same DUMP_SAMPLES flat indices (seeded, sorted) for the same shape in every run, saved
    beside it as DIR/<name>_index.npy (float64, exact) so that np.unravel_index(index, shape) places every value."""
    import numpy as np
    os.makedirs(outdir, exist_ok=True)
    total = 0
    for name, t in arrays.items():
        flat = t.detach().reshape(-1)
        if flat.numel() > DUMP_SAMPLES:
            idx = np.sort(np.random.default_rng(0).choice(flat.numel(), DUMP_SAMPLES, replace=False))
            flat = flat[torch.from_numpy(idx).to(flat.device)]
            np.save(os.path.join(outdir, f"{name}_index.npy"), idx.astype(np.float64))
            total += idx.size * 8
        v = flat.float().cpu().numpy()
        np.save(os.path.join(outdir, f"{name}.npy"), v)
        total += v.nbytes
        mark(f"dumped {name}: shape {tuple(t.shape)}, {v.size} value(s)")
    assert total <= 64 << 20, f"--dump-outputs wrote {total} bytes"


def prepare_gpu_run(a, dev):
    """Workload, eager warm-up, hipGraph capture and the two-stream pipeline -> (run, single_run, graphed, pipelined, engine, x0, sched, step)."""
    step, engine, agent, x0, sched = build_workload(a, dev)

    run = step
    single_run = None
    graphed = pipelined = False
    step()                                   # eager warm-up: lazy module init, MIOpen/rocBLAS plans
    torch.cuda.synchronize()
    if not a.no_graph:
        try:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                step()
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                step()
            run, graphed = graph.replay, True
            single_run = graph.replay
            if not a.no_pipeline:
                modes = ["interleaved", "streams"] if getattr(a, "pipeline", "streams") == "interleaved" else ["streams"]
                for mode in modes:
                    try:
                        prime, prun = (build_interleaved if mode == "interleaved" else build_pipeline)(step, engine, x0)
                        prime()
                        prun(); prun()
                        torch.cuda.synchronize()
                        run, pipelined = prun, mode
                        break
                    except Exception as e:
                        print(f"[bench] {mode} pipeline unavailable ({type(e).__name__}: {e})", file=sys.stderr)
                        torch.cuda.synchronize()
        except Exception as e:          # stays on the HIP kernels either way; only the launch mechanism differs
            print(f"[bench] hipGraph capture unavailable ({type(e).__name__}: {e}); launching eagerly", file=sys.stderr)
            torch.cuda.synchronize()
            run = step
    return run, single_run, graphed, pipelined, engine, x0, sched, step


def main():
    a = parse()
    if a.cpu_probe:
        return cpu_probe(a, a.cpu_probe)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` (how the driver calls it): this process has not touched the GPU and never will — it
        # starts one rank per GPU under torch.distributed.run as a CHILD, relays rank 0's JSON line (inherited stdout) and
        # exits with the child's code. (Replacing a GPU-initialised process by exec is what this pool forbids; we do neither.)
        from adaptiveisp_amd.dist import launch_ranks
        raise SystemExit(launch_ranks(a.gpus, os.path.abspath(__file__), sys.argv[1:]))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        raise SystemExit(f"bench.py: --gpus {a.gpus} but WORLD_SIZE={world}: launch one rank per GPU (or let --gpus N do it)")
    # BENCH_REHEARSAL=1: run the N-rank code path on a box with ONE GPU (every rank on device 0, gloo instead of RCCL, which
    # refuses two ranks on one device) — a rehearsal of the launch / barrier / max-over-ranks / rank-0-only logic, its
    # throughput means nothing and the JSON line says so. BENCH_REHEARSAL=dry: the same harness with NO device at all (the
    # step is a host sleep) — what tests/test_dist_gloo.py runs on the CPU box to pin `--gpus N` -> N ranks -> one line.
    rehearsal = os.environ.get("BENCH_REHEARSAL", "")
    dry = rehearsal == "dry"
    rehearsal = rehearsal in ("1", "dry")
    if dry:
        if a.dump_outputs:
            raise SystemExit("bench.py: --dump-outputs needs the device (a dry rehearsal computes nothing)")
        dev = torch.device("cpu")
    else:
        if not torch.cuda.is_available():
            raise SystemExit("bench.py needs a HIP device (the product has no CPU path)")
        if not rehearsal and torch.cuda.device_count() < world:
            raise SystemExit(f"bench.py: --gpus {world} but only {torch.cuda.device_count()} device(s) visible")
        if rehearsal:
            local = 0
        torch.cuda.set_device(local)
        dev = torch.device("cuda", local)
    dist = None
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    def barrier():
        if dist is not None:
            dist.barrier()
        if not dry:
            torch.cuda.synchronize()

    if dry:
        run, sched, Hp = (lambda: time.sleep(0.002)), SCHEDULES[a.schedule], (a.height + 31) // 32 * 32
        graphed = pipelined = False
        single_run = engine = x0 = step = None
        a.no_detail = a.no_cpu_baseline = True
    else:
        mark("building the workload: engine, eager step, hipGraph capture")
        run, single_run, graphed, pipelined, engine, x0, sched, step = prepare_gpu_run(a, dev)
        Hp = engine.Hp
    mark("workload built; warm-up")
    for _ in range(a.warmup):
        run()
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        run()
    barrier()
    dt = time.perf_counter() - t0
    mark(f"timed region done: {dt / a.steps * 1e3:.3f} ms per step")
    if engine is not None:
        engine.check_chains(sync=True)           # a chain wait that gave up = a wrong forward inside the timed region: raise
    if a.dump_outputs and rank == 0:
        # before the detail passes below reuse these buffers: the detections of the last timed step (engine.pred, what step()
        # returns) and the ISP image that step wrote (pipelined: the hand-over buffer of the next batch, the same input)
        isp_out = run.xbuf[(run.state["i"] - 1) & 1] if pipelined else step.isp_out
        dump_outputs(a.dump_outputs, {"detections": engine.pred, "isp_output": isp_out})
    if dist is not None:
        t = torch.tensor([dt], device=dev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    value = world * a.batch * a.steps / dt

    if os.environ.get("BENCH_EXPERIMENT_NO_POLICY") == "1":
        print(f"[bench] EXPERIMENT (policy launches cached: NOT the benchmark's step): {dt / a.steps * 1e3:.3f} ms per step", flush=True)
        return
    line = {
        "metric": f"ISP+YOLO forward images/sec @{a.width}x{a.height} bs{a.batch}", "value": round(value, 2), "unit": "images/sec",
        "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": round(dt / a.steps * 1e3, 3),
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
        "launch_mode": (pipelined if pipelined == "interleaved" else "pipelined") if pipelined else ("graph" if graphed else "eager"),
        "config": {"workload": f"batch {a.batch} x {a.width}x{a.height} " + ("uint16 RGGB Bayer plane -> demosaic -> " if a.raw else "") +
                               f"fp32 RGB, {len(sched)}-step ISP schedule "
                               f"{[NAMES[k] for k in sched]} (teacher-forced, policy/heads evaluated every step) + YOLOv3 "
                               f"forward @{a.width}x{Hp} bf16 (random-init weights)",
                   "per_gpu_batch": a.batch, "global_batch": a.batch * world, "parallelism": f"replicas x{world}",
                   "launch": ("hipGraph replay, 2-stage pipeline: the ISP episode of batch i+1 inside the detector forward of batch i — "
                              "its filter launches between the detector's layers on one stream, its policy launches on a second "
                              "(every step = one full ISP pass + one full detector pass)") if pipelined == "interleaved" else
                             ("hipGraph replay, 2-stage pipeline: one ISP episode's worth of steps (batch i+1 from its NLM "
                              "step on, then the first steps of batch i+2) beside the detector of batch i "
                              "(two streams; every step = one full ISP pass + one full detector pass)") if pipelined
                   else ("hipGraph replay" if graphed else "eager")},
    }
    if rank == 0 and pipelined and single_run is not None and not a.no_detail:
        # the same K steps without the cross-batch overlap (one stream: each detector pass waits for its own ISP episode)
        for _ in range(a.warmup):
            single_run()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for _ in range(a.steps):
            single_run()
        torch.cuda.synchronize()
        dt1 = time.perf_counter() - t1
        line["single_stream"] = {"value": round(a.batch * a.steps / dt1, 2), "unit": "images/sec", "n_gpus": 1,
                                 "ms_per_step": round(dt1 / a.steps * 1e3, 3)}
    if rank == 0 and pipelined and not a.no_detail:
        # the same K steps with the op ids read from the DEVICE by the filter launches (what a policy-selected evaluation
        # issues: adaisp_forward's per-family launches + the selective pooling launch) instead of the host-known op
        step.mode["device_ids"] = True
        try:
            dprime, drun = (build_interleaved if pipelined == "interleaved" else build_pipeline)(step, engine, x0)
            dprime()
            for _ in range(max(a.warmup, 2)):
                drun()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            for _ in range(a.steps):
                drun()
            torch.cuda.synchronize()
            dt2 = time.perf_counter() - t2
            line["device_selected_path"] = {"value": round(a.batch * a.steps / dt2, 2), "unit": "images/sec", "n_gpus": 1,
                                            "ms_per_step": round(dt2 / a.steps * 1e3, 3),
                                            "note": "same schedule delivered through device-side op ids (adaisp_forward), pipelined"}
            del dprime, drun
        except Exception as e:                               # noqa: BLE001
            line["device_selected_path"] = {"error": f"{type(e).__name__}: {e}"}
        finally:
            step.mode["device_ids"] = False
    if rank == 0 and not a.no_detail:
        runner = None
        if pipelined:
            mprime, runner = (build_interleaved(step, engine, x0, eager=True) if pipelined == "interleaved" else
                              build_pipeline(step, engine, x0, detector_eager=True))
            mprime()
            runner(); runner()
            torch.cuda.synchronize()
        mark("per-kernel conv timing")
        d = time_conv_kernels(engine, x0, runner=runner)
        mark("per-kernel conv timing done")

        at_baseline = (a.batch, a.height, a.width) == (8, 720, 1280)

        def roof(r):
            traffic, src = pmc_traffic(r["kernel"]) if at_baseline else (None, None)
            ref_ms, ref_src = rocprof_reference(r["kernel"]) if at_baseline else (None, None)
            return {"bound": "mfma", "kernel": r["kernel"], "achieved": round(r["tflops"], 1), "peak": MFMA_BF16_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(r["tflops"] / MFMA_BF16_PEAK_TFLOPS, 4),
                    # the same kernel with the detector ALONE on the chip (no NLM workgroups time-slicing its CUs): kernel
                    # quality, where `achieved` / `frac` are the figure inside the headline's two-stream arrangement
                    "achieved_clean": round(r["tflops_clean"], 1), "frac_clean": round(r["tflops_clean"] / MFMA_BF16_PEAK_TFLOPS, 4),
                    # separate --pmc passes of this workload, committed under profiles/ (not observed by THIS run); only for
                    # the BASELINE config's launch sizes
                    "traffic": traffic, "traffic_source": src,
                    "avg_launch_ms": round(r["avg_launch_ms"], 4), "avg_launch_ms_pipelined": round(r["avg_launch_ms"], 4),
                    "avg_launch_ms_clean": round(r["avg_launch_ms_clean"], 4), "launches_per_step": r["launches_per_step"],
                    "flops_per_launch": r["flops_per_launch"], "share_of_conv_time": round(r["share_of_conv_time"], 3),
                    # the committed profile of the same command (graph replay, both streams inside one graph): its average
                    # includes the few launches that time-slice a CU with an NLM workgroup (std dev ~ the mean)
                    "rocprof_avg_launch_ms": round(ref_ms, 4) if ref_ms else None, "rocprof_source": ref_src}

        # Which kernel the top-level `roofline` names: the TOP ROW of the committed rocprofv3 summary of this command when it is
        # one of the detector's conv kernels (so the fraction cannot move because kernels were re-partitioned and the live
        # shares of three near-equal kernels swapped places: VERDICT r5 weak #7); the largest live share otherwise
        dom, dom_rule = d["kernels"][0], "largest live share of conv time"
        top = rocprof_top_conv_kernel(d["kernels"]) if at_baseline else None
        if top is not None:
            dom, dom_rule = top, "top row of the committed rocprofv3 kernel stats"
        line["roofline"] = roof(dom)
        line["roofline"]["chosen_by"] = dom_rule
        # ... and the WHOLE detector against the same roof (all launches of one forward, detector alone on the chip): the figure
        # that moves only when the detector gets faster
        line["roofline"]["detector"] = {"ms": round(d["detector_ms"], 3), "tflops": round(d["detector_tflops"], 1),
                                        "frac": round(d["detector_tflops"] / MFMA_BF16_PEAK_TFLOPS, 4),
                                        "flops_per_forward": engine.flops, "peak": MFMA_BF16_PEAK_TFLOPS, "unit": "TFLOP/s"}
        line["roofline"]["measured"] = (f"HIP event pair around every launch, in the network, {d['reps']} forwards; avg_launch_ms = " +
                                        ("in the headline's arrangement (next batch's ISP filters between the layers, its policy on a "
                                         "second stream)" if pipelined == "interleaved" else
                                         "beside the ISP episode of the next batch on a second stream (the headline's arrangement)"
                                         if pipelined else "single stream") + "; *_clean = detector alone")
        line["roofline"]["other_kernels"] = [roof(r) for r in d["kernels"] if r is not dom][:3]
        # live figures vs the committed rocprofv3 summary of the same command. rocprofv3 times a dispatch from its first
        # workgroup's start to its last one's end; an event pair on the stream also contains the time a launch WAITS for CUs —
        # in the two-stream arrangement the detector's first small launches queue behind NLM's workgroups (3 x 48.5 KB of LDS
        # per CU leave no room for a conv workgroup), so their pipelined figure is wait + run while `clean` is run only. A
        # kernel is a violation when NEITHER live figure is within 25 % of the profile; `queued` lists the kernels whose
        # pipelined figure is > 1.5 x the clean one (contention, not kernel time)
        off, queued = [], []
        for r in [line["roofline"]] + line["roofline"]["other_kernels"]:
            ref = r.get("rocprof_avg_launch_ms")
            if r["avg_launch_ms"] > 1.5 * r["avg_launch_ms_clean"]:
                queued.append({"kernel": r["kernel"], "pipelined_ms": r["avg_launch_ms"], "clean_ms": r["avg_launch_ms_clean"]})
            if ref and min(abs(r["avg_launch_ms"] - ref), abs(r["avg_launch_ms_clean"] - ref)) > 0.25 * ref:
                off.append({"kernel": r["kernel"], "pipelined_ms": r["avg_launch_ms"], "clean_ms": r["avg_launch_ms_clean"],
                            "rocprof_ms": ref, "source": r["rocprof_source"]})
        line["consistency"] = {"ok": not off, "rule": "a live avg launch (pipelined or clean) within 25 % of the committed rocprofv3 avg",
                               "violations": off, "queued_behind_isp": queued}
        if off:
            print(f"[bench] CONSISTENCY: live per-kernel timings differ from the committed rocprofv3 summary by > 25 %: {off}",
                  file=sys.stderr)
        line["detector"] = {"ms": round(d["detector_ms"], 3), "tflops": round(d["detector_tflops"], 1),
                            "gflop_per_image": round(engine.flops / a.batch / 1e9, 1)}
        line["isp"] = {"bound": "hbm", "peak_GBps": HBM_PEAK_GBS, "bytes_per_px": 24,
                       "note": "ms/GBps: rotating buffers (HBM); warm_*: one buffer pair repeated (partly Infinity Cache); with_pool_ms: the RL step's launch incl. the next step's 64x64 pooling",
                       "kernels": time_isp_kernels(x0, sched)}
    if rank == 0 and world == 1 and not dry and not a.no_extras and not a.no_detail and \
            (a.batch, a.height, a.width, a.schedule) == (8, 720, 1280, "mixed"):
        mark("h2d")
        line["h2d"] = measure_h2d(a, dev, run, dt / a.steps * 1e3)
        mark("extras")
        del run, single_run, step, engine, x0
        run_extras(dev, line)
    if rank == 0 and not a.no_cpu_baseline and world == 1:
        mark("cpu_baseline")
        try:
            line["cpu_baseline"] = cpu_baseline(a, sched)
        except Exception as e:
            line["cpu_baseline"] = {"error": f"{type(e).__name__}: {e}"}
    if rehearsal:
        line["data"] = ("synthetic (DRY REHEARSAL: no device, the step is a host sleep; not a measurement)" if dry else
                        "synthetic (REHEARSAL: all ranks share one device; not a measurement)")
    if rank == 0:
        mark("done")
        print(json.dumps(line), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
