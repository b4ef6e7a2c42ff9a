"""N > 1 path on CPU (gloo, world sizes 2 and 4): the SHIPPING sharding / packing / gather code of rangedet_amd.dist, driven by
a real BatchPostProcessor (score filter + weighted NMS of the hipemu build) per rank -- frame f -> rank f % world, one
all_gather per step of the padded records, every rank ends up with every frame's detections; checked against the oracle."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _frame_inputs(f, n):
    """Frame f's (n,) scores and (n,10) boxes, rows sorted by score like the graph's outputs (cluster_dets -> 4 corners, z0, z1)."""
    from rangedet_amd import synth
    d = synth.cluster_dets(6 + f % 3, 7, seed=100 + f, quant=(64 if f % 2 else None))
    d = d[np.argsort(-d[:, 11], kind="stable")]
    sc = np.zeros(n, np.float32)
    bx = np.zeros((n, 10), np.float32)
    k = d.shape[0]
    sc[:k] = d[:, 11]
    bx[:k, :8], bx[:k, 8], bx[:k, 9] = d[:, :8], d[:, 9], d[:, 9] + d[:, 10]
    return sc, bx


def _worker(rank, world, port, nframes, B, out):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch.distributed as dist
    from emu_util import emu_lib, NumpyAllocator
    from rangedet_amd import dist as rdist
    from rangedet_amd.pipeline import BatchPostProcessor
    r, w = rdist.init_process_group("gloo")
    assert (r, w) == (rank, world)
    shard = rdist.FrameSharding()
    L, A = emu_lib(), NumpyAllocator()
    n, cap = 96, 64
    post = BatchPostProcessor(B, n, 0.5, 0.1, 0.5, False, L, A, cap)
    gat = rdist.DetectionGather(post, shard, A, L, max_det=16)
    seen = {}
    for step in range(shard.steps(nframes, B)):
        frames = shard.frames_of_step(step, B)
        sc = np.stack([_frame_inputs(f, n)[0] for f in frames])
        bx = np.stack([_frame_inputs(f, n)[1] for f in frames])
        post.enqueue_filter(sc.ctypes.data, n, bx.ctypes.data, n * 10)
        post.enqueue_nms()
        gat.enqueue()                                          # the one collective of the path
        seen.update(gat.unpack(step))
    # evaluate's per-rank dictionaries (record id -> result), merged on every rank
    from rangedet_amd import evaluate
    mine = shard.mine(nframes)
    ann, outd = evaluate.merge_across_ranks({f: None for f in mine}, {f: {"rank": rank} for f in mine})
    assert sorted(outd) == list(range(nframes)) and all(outd[f]["rank"] == f % world for f in outd) and sorted(ann) == sorted(outd)
    if rank == 0:
        out.put({f: (M, rows.tobytes()) for f, (rows, M) in seen.items()})
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 4])
def test_frame_sharding_and_gather_gloo(world):
    from oracle import cpu_ops as O
    from emu_util import emu_lib
    emu_lib()            # (build the CPU emulation of the HIP sources HERE if it is stale: minutes, which the workers' queue timeout would not survive)
    nframes, B = 8, 2 if world == 2 else 1
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, nframes, B, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = q.get(timeout=300)
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    steps = -(-(-(-nframes // world)) // B)
    assert sorted(got) == list(range(world * steps * B))       # every frame exactly once, all visible on rank 0
    for f in range(nframes):
        sc, bx = _frame_inputs(f, 96)
        dets = O.score_filter_to_dets(sc, bx, 0.5)
        flat, keep = O.wnms_4c(dets, 0.1, 0.5, False, 100)
        M, raw = got[f]
        rows = np.frombuffer(raw, np.float32).reshape(-1, 12)
        ref = np.array(flat, np.float32).reshape(-1, 12)
        assert M == len(keep) and rows.shape[0] == min(M, 16)
        assert np.array_equal(rows[:, [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]].view(np.uint32),
                              ref[:rows.shape[0]][:, [0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 11]].view(np.uint32))
        assert np.abs(rows[:, 8] - ref[:rows.shape[0], 8]).max() < 1e-5     # yaw column: atan2f of the score filter


def _late_worker(rank, world, port, out):
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import time
    import torch.distributed as dist
    from rangedet_amd import dist as rdist
    rdist.init_process_group("gloo")
    shard = rdist.FrameSharding()
    B, cap = 2, 32

    def make(step):
        class _Post:      # the fields of pipeline.BatchPostProcessor the gather reads
            pass
        post = _Post()
        post.B, post.cap = B, cap
        rows = np.zeros((B, cap, 12), np.float32)
        nk = np.zeros(B, np.int32)
        for j, f in enumerate(shard.frames_of_step(step, B)):
            nk[j] = 1 + f % 7
            rows[j, :nk[j]] = 100.0 * f + np.arange(nk[j], dtype=np.float32)[:, None]
        post.out, post.nkeep = rows.view(np.uint8).reshape(-1), nk.view(np.uint8)
        return rdist.DetectionGather(post, shard, rdist.HostAlloc, rdist.HostCopyLib, max_det=8), (rows, nk)
    dist.barrier()
    g0, keep0 = make(0)          # two pipelines' gathers, as bench.py / evaluate hold them
    g1, keep1 = make(1)
    if rank == 1:
        time.sleep(1.5)          # the late rank: its batch 0 is not ready yet
    t0 = time.perf_counter()
    g0.enqueue()                 # rank 0: its peer has not arrived -- the enqueue must return, ...
    t_enq0 = time.perf_counter() - t0
    g1.pack()                    # ... and so must the NEXT batch's (nothing queues up behind the first collective) -- in the two-call form
    g1.gather()                  #     the timed pipeline uses: pack behind the NMS, the collective once the pack's event has fired
    t_enq1 = time.perf_counter() - t0
    got0 = g0.unpack(0)          # only the harvest of batch 0 waits for the late rank
    t_done0 = time.perf_counter() - t0
    got1 = g1.unpack(1)
    ok = True
    for step, got in ((0, got0), (1, got1)):
        ok = ok and sorted(got) == sorted(f for r in range(world) for f in shard.frames_of_step(step, B, rank=r))
        for f, (rw, M) in got.items():
            ok = ok and M == 1 + f % 7 and np.array_equal(rw[:, 0], 100.0 * f + np.arange(M, dtype=np.float32))
    out.put((rank, t_enq0, t_enq1, t_done0, bool(ok)))
    dist.barrier()
    dist.destroy_process_group()


def test_gather_enqueue_does_not_wait_for_a_late_rank():
    """the collective lives on its own communication stream (GPU) / is asynchronous (host buffers): a rank whose
    peer is 1.5 s late gets both of its enqueues back at once; only the harvest (unpack) of that batch waits.  (tools/test.py:139-170
    has no collective at all -- its result queue never blocks a GPU thread.)"""
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_late_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = dict((r[0], r[1:]) for r in (q.get(timeout=120) for _ in range(world)))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    enq0, enq1, done0, ok = res[0]
    assert ok and res[1][3]
    assert enq0 < 0.5 and enq1 < 0.5, "rank 0's enqueues waited for the late rank: %.2f s, %.2f s" % (enq0, enq1)
    assert done0 > 1.0, "rank 0's harvest of batch 0 cannot complete before the late rank arrived (%.2f s)" % done0


def test_sharding_arithmetic():
    from rangedet_amd.dist import FrameSharding, record_floats
    s = FrameSharding(rank=3, world=8)
    assert s.frames_of_step(0, 8) == [3 + 8 * j for j in range(8)] and s.frames_of_step(2, 8)[0] == 3 + 8 * 16
    assert s.mine(20) == [3, 11, 19] and s.owner(19) == 3
    assert FrameSharding(0, 8).steps(64, 8) == 1 and FrameSharding(0, 8).steps(65, 8) == 2 and FrameSharding(0, 1).steps(5, 2) == 3
    assert record_floats() == 2401
    every = sorted(f for r in range(8) for st in range(2) for f in FrameSharding(r, 8).frames_of_step(st, 4))
    assert every == list(range(64))


@pytest.mark.parametrize("launcher", ["self", "torchrun"])
def test_bench_launches_itself(launcher):
    """`python bench.py --gpus 2` (the driver's command form) spawns its own two ranks when no launcher set RANK / WORLD_SIZE, and
    also runs under torch.distributed.run; RD_BENCH_DRYRUN keeps it to the launch / rendezvous / gather / report skeleton (gloo)."""
    import json
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["RD_BENCH_DRYRUN"] = "1"
    tail = [os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1"]
    if launcher == "self":
        cmd = [sys.executable] + tail
    else:
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
               "--master-port", str(_free_port())] + tail
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["ranks_seen"] == [0, 1] and d["n_gpus"] == 2 and d["frames_step0"] == list(range(16))
    # ... and the dry run drives the SHIPPING gather (dist.DetectionGather: pack, one all_gather, unpack) on host buffers: every rank
    # found all 16 frames of a step with the rows their owners wrote
    assert d["gather_ok"] is True and d["gathered_frames"] == 16


def test_rank_and_device_checks():
    """dist.check_ranks: anything but `world` distinct ranks on `world` distinct GPUs stops the run; dist.bind_cpus cuts the allowed
    CPU list into per-rank slices (reference: utils/cpu_affinity.py:38-47) and restores nothing it did not change."""
    from rangedet_amd import dist as rdist
    ids = [bytes([i]) * 16 for i in range(4)]
    rdist.check_ranks([0, 1, 2, 3], ids, 4)
    with pytest.raises(RuntimeError, match="ranks"):
        rdist.check_ranks([0, 1, 1, 3], ids, 4)
    with pytest.raises(RuntimeError, match="share a GPU"):
        rdist.check_ranks([0, 1, 2, 3], [ids[0], ids[1], ids[1], ids[3]], 4)
    before = os.sched_getaffinity(0)
    try:
        assert rdist.bind_cpus(0, 1) is None and os.sched_getaffinity(0) == before          # a single rank is left alone
        if len(before) >= 2:
            a = rdist.bind_cpus(1, 2)
            assert a == sorted(before)[len(before) // 2: 2 * (len(before) // 2)] and os.sched_getaffinity(0) == set(a)
    finally:
        os.sched_setaffinity(0, before)
    os.environ["RD_NO_AFFINITY"] = "1"
    try:
        assert rdist.bind_cpus(0, 2) is None
    finally:
        del os.environ["RD_NO_AFFINITY"]


def test_bench_world_mismatch_is_an_error_not_an_assert():
    import subprocess
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", RD_BENCH_DRYRUN="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=1" in r.stderr


def _json_line(stdout):
    import json
    lines = [ln for ln in stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, stdout[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_rccl_gather_world1():
    """The RCCL branch of bench.py on ONE GPU (RD_BENCH_GATHER=1): `init_process_group("nccl", device_id=...)`, the rank / device
    report through the communicator, `all_gather_into_tensor` of the padded detections on the post-processing stream behind the NMS,
    and the gathered records against what the rank put in and against the same run without the collective
    (replaces the per-GPU result queue of tools/test.py:139-170)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RD_BENCH_GATHER")}
    env["MASTER_PORT"] = str(_free_port())
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--repeats", "2", "--no-cpu-baseline"]
    plain = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert plain.returncode == 0, plain.stderr[-2000:]
    gath = subprocess.run(cmd, env=dict(env, RD_BENCH_GATHER="1"), capture_output=True, text=True, timeout=900)
    assert gath.returncode == 0, gath.stderr[-2000:]
    p, g = _json_line(plain.stdout), _json_line(gath.stdout)
    pc, gc = p["config"], g["config"]
    assert pc["rccl_version"] is None and pc["gathered_frames_last_step"] is None
    assert gc["ranks_seen"] == [0] and gc["rccl_version"] and gc["gathered_frames_last_step"] == 8
    assert gc["gather_matches_local"] is True                                  # the collective returned this rank's records bit for bit
    assert gc["results_sha256_last_step"] == pc["results_sha256_last_step"]    # ... and the results are those of the run without it
    assert gc["wnms_kept"] == pc["wnms_kept"] and gc["wnms_candidates"] == pc["wnms_candidates"]
    # the weighted NMS's rejection test (k_wnms.h w_pair_skippable) on the production frames -- the whole run again with every
    # pair clipped (bench.py --wnms-no-skip = the call's RD_WNMS_DIAG_NO_SKIP bit): the same kept rows and indices, bit for bit
    ns = subprocess.run(cmd + ["--wnms-no-skip"], env=env, capture_output=True, text=True, timeout=900)
    assert ns.returncode == 0, ns.stderr[-2000:]
    nc = _json_line(ns.stdout)["config"]
    assert nc["results_sha256_last_step"] == pc["results_sha256_last_step"] and nc["wnms_kept"] == pc["wnms_kept"]
    for d in (p, g):                                                           # the spread fields of the report
        assert d["roofline"] is None and d["meta_dla_forward"] is None and "cpu_baseline" not in d    # (a plain run: no --full replays)
        assert d["repeats"] == 2 and len(d["region_ms"]) == 2 and d["steps"] == 5
        assert d["ms_per_step_p5"] <= d["ms_per_step_p50"] <= d["ms_per_step_p95"]
        assert d["value_min"] <= d["value"] <= d["value_max"]


@pytest.mark.gpu
def test_evaluate_rccl_merge_world1(tmp_path):
    """`python -m rangedet_amd.evaluate` through its multi-rank branch with one rank (RD_EVAL_GATHER=1: nccl communicator bound to
    the GPU, sharded record list, per-rank dictionaries merged through the collective) writes the same pickle as the plain run."""
    import pickle
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "RD_EVAL_GATHER")}
    env["MASTER_PORT"] = str(_free_port())
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    outs = []
    for tag, extra in (("plain", {}), ("rccl", {"RD_EVAL_GATHER": "1"})):
        out = str(tmp_path / (tag + ".pkl"))
        r = subprocess.run([sys.executable, "-m", "rangedet_amd.evaluate", "--synthetic", "3", "--random-weights", "--batch", "2", "--gpus", "1", "--out", out],
                           env=dict(env, **extra), capture_output=True, text=True, timeout=900, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
        assert ("through the nccl communicator" in r.stdout) == (tag == "rccl"), r.stdout[-1000:]
        with open(out, "rb") as f:
            outs.append((pickle.load(f), pickle.load(f)))
    (a0, o0), (a1, o1) = outs
    assert sorted(o0) == sorted(o1) and len(o0) > 0 and sorted(a0) == sorted(a1)
    for k in o0:
        assert o0[k]["meta_info"] == o1[k]["meta_info"]
        for c in o0[k]["det_xyzlwhyaws"]:
            assert np.array_equal(o0[k]["det_xyzlwhyaws"][c], o1[k]["det_xyzlwhyaws"][c])


@pytest.mark.gpu
def test_bench_results_independent_of_block_fusion():
    """The timed pipeline itself -- three batches in flight on three launch streams, each with its NMS behind its forward, i.e. the fused BasicBlock
    kernels (csrc/k_block.h, counted LDS-DMA waits) running under contention -- gives bit for bit the detections of the same run with
    every block as its two launches (RD_NO_FUSE_BLOCK=1): digest of the last step's kept rows and indices of all 8 frames, and the digest over
    EVERY step's host results (120+ steps, warm-up included).  Two separate runs: so this is also the run-to-run determinism check of the
    whole pipeline under three batches in flight (it failed before the build dropped the swapped packed-fp32 form)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "RD_NO_FUSE_BLOCK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "3", "--repeats", "3", "--backbone-reps", "0",
           "--no-cpu-baseline", "--full"]
    outs = []
    for extra in ({}, {"RD_NO_FUSE_BLOCK": "1", "RD_DEV_SWITCHES": "1"}):
        r = subprocess.run(cmd, env=dict(env, **extra), capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        outs.append(_json_line(r.stdout))
    a, b = outs
    assert a["block_kernel"] is not None and a["block_kernel"]["launches_per_step"] == 8 and b["block_kernel"] is None
    assert a["config"]["results_sha256_last_step"] == b["config"]["results_sha256_last_step"]
    assert a["config"]["results_sha256_all_steps"] == b["config"]["results_sha256_all_steps"]      # every step's host results, warm-up included
    # ... and of the same steps with ONE batch in flight: what runs overlapped gives what runs alone
    r = subprocess.run(cmd + ["--inflight", "1"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    c = _json_line(r.stdout)
    assert c["config"]["results_sha256_all_steps"] == a["config"]["results_sha256_all_steps"]
    # ... and of the same steps replayed from hipGraphs (round 6, pipeline.RangeDetPipeline(graph=True): one graph per pipeline and input
    # set, ~80 launches per replay call), with three and with two batches in flight
    for extra_args in (["--graph"], ["--graph", "--inflight", "2"]):
        r = subprocess.run(cmd + extra_args, env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-2000:]
        g = _json_line(r.stdout)
        hg = g["config"]["hip_graph"]
        assert hg["graphs"] >= 2 and hg["replays"] >= 100, hg
        assert g["config"]["results_sha256_all_steps"] == a["config"]["results_sha256_all_steps"]
    # ... and of the same steps with every batch's inputs uploaded from pinned host memory in front of its forward (--h2d, the PCIe-inclusive
    # diagnostic: one device input set per pipeline, overwritten only after that pipeline's previous batch has been harvested)
    r = subprocess.run(cmd + ["--h2d"], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    u = _json_line(r.stdout)
    assert u["config"]["inputs"].startswith("uploaded every step") and a["config"]["inputs"].startswith("resident")
    assert u["config"]["results_sha256_all_steps"] == a["config"]["results_sha256_all_steps"]
    assert a["config"]["wnms_kept"] == b["config"]["wnms_kept"] > 0 and a["meta_dla_forward"] is None


@pytest.mark.gpu
def test_wnms_chain_unaffected_by_concurrent_convs():
    """Round 5: with two or more batches in flight the keep counts of a frame differed by one or two from run to run.  Cause: the SLP
    vectoriser's packed-fp32 form with a swapped second source (v_pk_mul_f32 ... op_sel:[0,1] op_sel_hi:[1,0]) returns a wrong low half in
    lanes 48-63 while another wave of the SIMD issues MFMA instructions (tools/micro/pkform_test.py).  The library is built
    without that form (rangedet_amd/build.py); here the batched NMS chain is replayed on one stream while 64->64 convolutions (two
    workgroups per CU, room left on every SIMD) run on another, and must reproduce the idle GPU's result every time.  (The old build
    failed 15 of 20 such replays.)"""
    import torch
    from rangedet_amd import lib as R, synth
    from rangedet_amd.pipeline import RangeDetPipeline
    B = 8
    P = synth.make_weights(seed=18)
    pipe = RangeDetPipeline(P, dtype=R.RD_BF16, batch=B, wnms_cap=8192)
    L, A, bp = pipe.lib, pipe.alloc, pipe.bpost
    pipe.enqueue(synth.make_batch(list(range(B)), lib=L, alloc=A))
    torch.cuda.synchronize()

    def snap():
        torch.cuda.synchronize()
        nk = np.array(A.to_numpy(A.view_i32(bp.nkeep, (B,))))
        keep = np.array(A.to_numpy(A.view_i32(bp.keep, (B, bp.cap))))
        rows = np.array(A.to_numpy(A.view_f32(bp.out, (B, bp.cap, 12))))
        return nk, [keep[b, :nk[b]].copy() for b in range(B)], [rows[b, :nk[b]].view(np.uint32).copy() for b in range(B)]

    def same(s, t):
        return np.array_equal(s[0], t[0]) and all(np.array_equal(a, b) for a, b in zip(s[1], t[1])) and all(np.array_equal(a, b) for a, b in zip(s[2], t[2]))

    bp.enqueue_nms()
    base = snap()
    assert int(base[0].min()) > 100
    bp.enqueue_nms()
    assert same(snap(), base)
    c, H, W = 64, 64, 2656
    x = torch.randn(B * H * W * c, device="cuda").to(torch.bfloat16)
    y = torch.empty_like(x)
    w = torch.from_numpy(L.pack_conv3x3_ex(np.random.RandomState(0).randn(c, c, 3, 3).astype(np.float32) * 0.05, 1, c, fold_scale=np.ones(c, np.float32),
                                           dtype=R.RD_BF16)).cuda()
    sh = torch.zeros(c, device="cuda")
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    bad = 0
    for _ in range(16):
        for _ in range(8):
            L.call("rd_conv3x3_bn_act_ex", x.data_ptr(), c, 0, w.data_ptr(), None, sh.data_ptr(), None, 0, 0, None, 0, 0, 0, None,
                   y.data_ptr(), c, 0, B, H, W, c, c, 1, R.RD_RELU_POST | R.RD_SCALE_FOLDED, R.RD_BF16, s1.cuda_stream)
        bp.enqueue_nms(stream=s2)
        bad += not same(snap(), base)
    assert bad == 0, "%d of 16 replays next to the convolutions differ from the idle result" % bad


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [["--config", "kitti", "--dtype", "f16"], ["--dtype", "f16"], ["--inflight", "1"]], ids=["kitti-f16", "waymo-f16", "inflight1"])
def test_bench_other_configurations_run(extra):
    """`bench.py` on the other configurations it names -- BASELINE configs[4] (KITTI-shaped two-class, fp16), the reference's arithmetic type
    on the headline workload, one batch in flight -- prints a well-formed line (the driver only ever runs the default)."""
    import subprocess
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "2", "--repeats", "2", "--no-cpu-baseline",
           "--full"] + extra
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _json_line(r.stdout)
    assert d["value"] > 100 and d["unit"] == "frames/s" and d["n_gpus"] == 1 and d["steps"] == 4 and d["repeats"] == 2
    assert d["dtype"] == ("f16" if "f16" in extra else "bf16") and d["roofline"]["frac"] > 0.2 and d["block_kernel"]["launches_per_step"] == 8
    assert 0.2 < d["meta_dla_forward"]["frac_hbm_peak"] < 0.6 and d["config"]["wnms_kept"] > 0
    if "kitti" in extra:
        assert "KITTI" in d["config"]["workload"] and set(d["config"]["per_class"]) == {"veh", "ped"}
