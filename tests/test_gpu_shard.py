"""Single-process multi-rank shard context of the C ABI (csrc/shard.hip) on ONE GPU: the same device listed 2 or 3 times selects the
copy transport (hipMemcpyAsync + events instead of RCCL) with identical packing and summation, so the whole N-rank flow of
mdtile/sharding.py::ShardedBlend -- band partition, per-rank partial blends, halo exchange, finalize, region ownership -- is
checked against the single-device blend.  (The RCCL transport itself needs distinct devices: exercised by bench.py --gpus N.)"""
import pytest
import torch

from oracle import blend_oracle as bo

pytestmark = pytest.mark.gpu


def _tile_fn(t):
    return 0.9 * t + 0.1 * t.flip(-1)


def _region_fn(t, k):
    return (0.8 - 0.05 * k) * t + 0.2 * t.flip(-2)


@pytest.mark.parametrize("world", [2, 3])
def test_halo_exchange_sums_in_rank_order(plugin, cuda, world):
    E = plugin.engine
    from mdtile import sharding
    sh = E.Shard(dev_ids=[0] * world)
    assert (sh.nranks, sh.nlocal, sh.rccl) == (world, world, False)
    H, W, N, C = 96, 40, 2, 4
    ys = [0, 20, 40, 60]                         # 4 tile rows of height 36: neighbours overlap by 16 rows
    bands = sharding.band_partition(ys, 36, 3, H, world)
    table = sharding.band_rows_table(bands)
    torch.manual_seed(world)
    parts = [torch.randn(N, C, H, W, device=cuda) for _ in range(world)]
    ref = [p.clone() for p in parts]
    for r in range(world):                        # restatement: shared rows = sum of every toucher's piece, ascending rank
        for y in range(bands[r].row_lo, bands[r].row_hi):
            touch = [q for q in range(world) if bands[q].row_lo <= y < bands[q].row_hi]
            if len(touch) > 1:
                acc = parts[touch[0]][:, :, y].clone()
                for q in touch[1:]:
                    acc = acc + parts[q][:, :, y]
                ref[r][:, :, y] = acc
    scratch = sh.halo_scratch(table, N, C, W)
    sh.halo_exchange(parts, scratch, table, streams=[torch.cuda.current_stream().cuda_stream] * world)
    torch.cuda.synchronize()
    for r in range(world):
        lo, hi = bands[r].row_lo, bands[r].row_hi
        assert torch.equal(parts[r][:, :, lo:hi], ref[r][:, :, lo:hi])
    bufs = [torch.full((5,), float(r + 1), dtype=torch.float64, device=cuda) for r in range(world)]
    sh.allreduce_stats(bufs)
    assert all(torch.equal(b.cpu(), torch.full((5,), float(sum(range(1, world + 1))), dtype=torch.float64)) for b in bufs)


REGIONS = [(4, 6, 30, 20, "Background", 0.2), (20, 30, 36, 28, "Foreground", 0.4), (0, 50, 24, 30, "Background", 0.2)]


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("with_regions", [False, True])
def test_sharded_blend_matches_single_device(plugin, cuda, world, method, with_regions):
    """cfg5 shape class: grid + region prompt control, tiles in row bands and regions dealt to the ranks."""
    E = plugin.engine
    from mdtile import sharding
    W, H, tw, th, ov, bs, N, C = 64, 96, 32, 32, 12, 4, 2, 4
    M = E.METHOD_MD if method == "md" else E.METHOD_MOD
    regs = [(x, y, w, h, E.REGION_BG if mode == "Background" else E.REGION_FG, fr) for (x, y, w, h, mode, fr) in REGIONS] if with_regions else []
    torch.manual_seed(5)
    x = torch.randn(N, C, H, W, device=cuda)
    # single-device reference through the same engine calls the delegates make
    one = sharding.ShardedBlend(E.Shard(dev_ids=[0]), W, H, tw, th, ov, bs, M, regions=regs)
    ref = one.step([x], _tile_fn, _region_fn)[0].clone()
    o = bo.BlendOracle(method, W, H, tw, th, ov, bs, [bo.Region(*r) for r in (REGIONS if with_regions else [])], True)
    want = o.evaluate(x.cpu(), _tile_fn, _region_fn)
    assert torch.allclose(ref.cpu(), want, rtol=1e-5, atol=1e-6), "one-rank ShardedBlend vs the oracle"
    sb = sharding.ShardedBlend(E.Shard(dev_ids=[0] * world), W, H, tw, th, ov, bs, M, regions=regs)
    outs = sb.allgather_rows(sb.step([x.clone() for _ in range(world)], _tile_fn, _region_fn))
    for r, out in enumerate(outs):
        assert torch.allclose(out, ref, rtol=1e-5, atol=1e-6), f"rank {r} of {world}: max diff {(out - ref).abs().max().item()}"
    # rows touched by one band only carry exactly the single-device value (same kernel, same order)
    for r, b in enumerate(sb.bands):
        if b.empty:
            continue
        solo = [y for y in range(b.row_lo, b.row_hi) if sum(1 for q in sb.bands if not q.empty and q.row_lo <= y < q.row_hi) == 1]
        if solo and not with_regions:
            assert torch.equal(outs[r][:, :, solo], ref[:, :, solo])


def _tile_fn_f32_inside(t):
    """_tile_fn evaluated in fp32 and rounded once to the I/O dtype (for fp32 tensors: _tile_fn itself)."""
    return _tile_fn(t.float()).to(t.dtype)


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("method", ["md", "mod"])
@pytest.mark.parametrize("dt", ["f32", "f16"])
@pytest.mark.parametrize("geom", ["odd200", "odd3rows"])
def test_sharded_blend_odd_origins_matches_single_device(plugin, cuda, world, method, dt, geom):
    """test_sharded_blend_matches_single_device on grids with odd tile origins (tile 96 / overlap 48: origins 0, 34, 69, 104), where every
    band's launch -- tile range + partial sums + row band over the packed buffer -- is a k_blend_lds launch (asserted through the dispatch
    query), in fp32 and fp16; two tile rows (the third of 3 ranks stays empty) and three.
    Rows owned by one band: bitwise the one-rank result.  Rows shared by bands are summed across ranks in another order than the one-rank
    list order: fp32 keeps that test's rtol = 1e-5, atol = 1e-6.  fp16 stores each of the two fp32 values with one rounding to nearest,
    an error of at most half an fp16 ulp each, ulp(v) <= 2^-10 |v| for normal v and 2^-24 below: rtol = 1e-5 + 2^-10, atol = 1e-6 + 2^-24."""
    import blend_matrix_cases as bm
    E = plugin.engine
    from mdtile import sharding
    W, H, tw, th, ov, bs = bm.GEOMETRIES[geom]
    N, C = 2, 4
    dtype = torch.float32 if dt == "f32" else torch.float16
    rtol, atol = (1e-5, 1e-6) if dt == "f32" else (1e-5 + 2.0 ** -10, 1e-6 + 2.0 ** -24)
    M = E.METHOD_MD if method == "md" else E.METHOD_MOD
    label = next(c for c in bm.SHARD_CASES if (c.geom, c.dtype, c.method) == (geom, dt, method))
    torch.manual_seed(5)
    x = torch.randn(N, C, H, W).to(dtype).to(cuda)
    one = sharding.ShardedBlend(E.Shard(dev_ids=[0]), W, H, tw, th, ov, bs, M)
    ref = one.step([x], _tile_fn_f32_inside)[0].clone()
    o = bo.BlendOracle(method, W, H, tw, th, ov, bs)
    want = o.evaluate(x.cpu().float(), lambda t: _tile_fn_f32_inside(t.to(dtype)).float()).to(dtype)
    assert torch.allclose(ref.cpu().float(), want.float(), rtol=rtol, atol=atol), "one-rank ShardedBlend vs the oracle"
    sb = sharding.ShardedBlend(E.Shard(dev_ids=[0] * world), W, H, tw, th, ov, bs, M)
    live = [b for b in sb.bands if not b.empty]
    assert len(live) == min(world, sb.local[0]["plan"].rows)
    for b in live:       # the launch ShardedBlend.step makes for this band
        d = E.blend_dispatch(sb.local[0]["plan"], dtype, N, C, packed=True, partial=True, tile_range=(b.tile_lo, b.tile_hi), row_range=(b.row_lo, b.row_hi))
        assert label.kernel == "lds" and d.lds and d.planes == label.lpp, f"band of rank {b.rank}: {d}"
    outs = sb.allgather_rows(sb.step([x.clone() for _ in range(world)], _tile_fn_f32_inside))
    for r, out in enumerate(outs):
        assert out.dtype == dtype
        assert torch.allclose(out.float(), ref.float(), rtol=rtol, atol=atol), f"rank {r} of {world}: max diff {(out.float() - ref.float()).abs().max().item()}"
    checked = 0
    for r, b in enumerate(sb.bands):
        if b.empty:
            continue
        solo = [y for y in range(b.row_lo, b.row_hi) if sum(1 for q in sb.bands if not q.empty and q.row_lo <= y < q.row_hi) == 1]
        if solo:
            assert torch.equal(outs[r][:, :, solo].view(torch.int32 if dt == "f32" else torch.int16),
                               ref[:, :, solo].view(torch.int32 if dt == "f32" else torch.int16)), f"rank {r}: solo rows differ bitwise"
            checked += len(solo)
    assert checked > 0


def test_vae_multi_device_sweep_matches_single_device(plugin, cuda):
    """VAEHook.devices: single-process multi-device decode (tiles dealt round-robin, per-device packed weights and streams, output
    rectangles copied to the first device).  Listing cuda:0 twice runs the whole flow on one GPU; the result must equal the ordinary
    sweep bit for bit (same kernels, same frozen statistics)."""
    from hostsim import ldm_decoder as ld
    dec = ld.make_decoder(4).to(cuda)
    dec.original_forward = dec.forward
    torch.manual_seed(13)
    z = torch.randn(1, 4, 40, 52, device=cuda)
    hook = plugin.tilevae.VAEHook(dec, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    one = hook(z).clone()
    hook.devices = [0, 0, 0]
    many = hook(z)
    assert many.device == one.device and torch.equal(many, one)


# ---- process-per-GPU bring-up with the seat belt (bench.py at N > 1) -------------------------------------------------------
def _free_port() -> int:
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _ctx_worker(rank, world, port, q):
    import os
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "multidiffusion-upscaler-for-automatic1111_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=rank, world_size=world)
        from mdtile import sharding
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        active = sharding.init_process_context_checked(rank, world, 0, timeout_s=60.0)
        # whichever transport survived, the exchange must give the rank-ordered sum on this band's rows
        rows = 8 * world
        bands = [sharding.Band(r, r, r + 1, r, r + 1, max(0, 8 * r - 3), min(rows, 8 * r + 11), 8 * r, 8 * r + 8) for r in range(world)]
        parts = [torch.randn(2, 4, rows, 32, generator=torch.Generator().manual_seed(50 + r)) for r in range(world)]
        mine = parts[rank].to(dev)
        sharding.exchange_and_sum(mine, bands, rank)
        lo, hi = bands[rank].row_lo, bands[rank].row_hi
        want = torch.zeros(2, 4, rows, 32)
        for r in range(world):                              # ascending rank order, contributors only
            b = bands[r]
            a, e = max(lo, b.row_lo), min(hi, b.row_hi)
            if a < e:
                want[:, :, a:e] += parts[r][:, :, a:e]
        ok = torch.equal(mine.cpu()[:, :, lo:hi], want[:, :, lo:hi])
        q.put((rank, bool(active), ok, ""))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        q.put((rank, None, False, repr(e)))


def test_process_context_bringup_agrees_and_exchanges(plugin, cuda):
    """Two processes on cuda:0 (gloo rendezvous): RCCL cannot put two ranks on one device, so the checked bring-up must end
    in the SAME state on both ranks -- normally 'fall back to torch.distributed' -- and the exchange must still be exact."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_ctx_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(60)
    assert all(r[3] == "" for r in res), res
    assert res[0][1] == res[1][1], f"ranks disagree about the transport: {res}"
    assert all(r[2] for r in res), res


# ---- RCCL itself, on the hardware at hand: a ONE-rank communicator through the product path ----------------------------------
def test_rccl_one_rank_communicator_process_form(plugin, cuda):
    """mdtile_shard_unique_id -> mdtile_shard_init_rank(nranks = 1): dlopen of librccl, the symbol table, ncclCommInitRank, then every
    collective the engine issues (ncclAllReduce, ncclBroadcast, a grouped self ncclSend / ncclRecv, ncclAllGather) on torch's stream."""
    E = plugin.engine
    sh = E.Shard(nranks=1, rank=0, uid=E.Shard.unique_id(), device=0)
    assert (sh.nranks, sh.nlocal, sh.first, sh.rccl) == (1, 1, 0, True)
    sh.selfcheck()                                                   # the engine's own bring-up check (context streams)
    cur = [torch.cuda.current_stream().cuda_stream]
    d = torch.arange(8, dtype=torch.float64, device=cuda) * 0.5
    want = d.clone()
    sh.allreduce_stats([d], streams=cur)
    b = torch.randn(1000, device=cuda)
    bw = b.clone()
    sh.bcast([b], 0, streams=cur)
    snd = torch.randn(3, 4096, device=cuda)
    rcv = torch.zeros_like(snd)
    sh.p2p([[(0, snd, rcv)]], streams=cur)                            # grouped self send / receive
    g = sh.allgather([snd], streams=cur)[0]
    torch.cuda.synchronize()
    assert torch.equal(d, want) and torch.equal(b, bw) and torch.equal(rcv, snd) and torch.equal(g[0], snd)
    sh.destroy()


def test_rccl_one_rank_communicator_single_process_form(plugin, cuda, monkeypatch):
    """mdtile_shard_init(1, {0}) with MDTILE_SHARD_TRANSPORT=rccl: ncclCommInitAll on one device (a one-device context normally
    needs no transport and takes the copy path)."""
    E = plugin.engine
    monkeypatch.setenv("MDTILE_SHARD_TRANSPORT", "rccl")
    sh = E.Shard(dev_ids=[0])
    assert (sh.nranks, sh.nlocal, sh.rccl) == (1, 1, True)
    sh.selfcheck()
    sh.destroy()
    monkeypatch.delenv("MDTILE_SHARD_TRANSPORT")
    assert E.Shard(dev_ids=[0]).rccl is False


@pytest.mark.parametrize("world", [1, 2, 3])
def test_selfcheck_p2p_allgather_copy_transport(plugin, cuda, world):
    """The same bring-up check and the generic collectives on the copy transport (one GPU listed `world` times)."""
    E = plugin.engine
    sh = E.Shard(dev_ids=[0] * world)
    assert sh.rccl is False
    sh.selfcheck()
    torch.manual_seed(world)
    cur = [torch.cuda.current_stream().cuda_stream] * world
    # every rank sends a distinct row to every other rank; the k-th send to a peer pairs with the peer's k-th receive from me
    payload = [[torch.randn(257, device=cuda) for _ in range(world)] for _ in range(world)]       # payload[src][dst]
    inbox = [[torch.zeros(257, device=cuda) for _ in range(world)] for _ in range(world)]         # inbox[dst][src]
    ops = [[(q, payload[r][q], inbox[r][q]) for q in range(world) if q != r] for r in range(world)]
    if world > 1:
        sh.p2p(ops, streams=cur)
    parts = sh.allgather([payload[r][r] for r in range(world)], streams=cur)
    torch.cuda.synchronize()
    for r in range(world):
        for q in range(world):
            if q != r:
                assert torch.equal(inbox[r][q], payload[q][r])
            assert torch.equal(parts[r][q], payload[q][q])


def _ctx1_worker(port, q):
    import os
    import sys
    import torch.distributed as dist
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "multidiffusion-upscaler-for-automatic1111_amd")):
        if p not in sys.path:
            sys.path.insert(0, p)
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        dist.init_process_group("gloo", rank=0, world_size=1)
        from mdtile import sharding
        dev = torch.device("cuda:0")
        torch.cuda.set_device(dev)
        active = sharding.init_process_context_checked(0, 1, 0, timeout_s=120.0)
        ctx = sharding.process_context()
        t = torch.arange(6, dtype=torch.float32, device=dev)
        r = sharding.comm_allreduce_sum(t.clone())
        parts = sharding.comm_allgather(t, 1)
        snd, rcv = t.clone(), torch.zeros_like(t)
        sharding.comm_p2p([(0, snd, rcv)])
        torch.cuda.synchronize()
        ok = torch.equal(r, t) and torch.equal(parts[0], t) and torch.equal(rcv, snd)
        q.put((bool(active), ctx is not None and ctx.rccl, bool(ok), ""))
        dist.destroy_process_group()
    except BaseException as e:  # noqa: BLE001
        q.put((None, None, False, repr(e)))


def test_process_context_bringup_one_rank_uses_rccl(plugin, cuda):
    """bench.py's N > 1 bring-up (gloo control group + the engine's own RCCL communicator for the data plane) with world = 1:
    the checked bring-up must END on the C-ABI context and the data-plane helpers must run on it."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    p = ctx.Process(target=_ctx1_worker, args=(_free_port(), q))
    p.start()
    res = q.get(timeout=300)
    p.join(60)
    assert res[3] == "", res
    assert res[0] is True and res[1] is True and res[2] is True, res


@pytest.mark.parametrize("world", [2, 3, 4])
def test_bench_flow_n_ranks_on_one_device_matches_the_single_rank_image(cuda, world):
    """The complete N-rank bench flow -- tile-row bands + halo exchange of the blend, sequence-parallel estimator, VAE tiles dealt to the
    ranks, decoded rectangles gathered to rank 0 inside the step -- as `world` processes sharing cuda:0 over gloo (host-staged transport:
    two RCCL ranks cannot sit on one device), on a 2048 x 2048 image at decoder tile 64 (16 tiles; world = 4: more ranks than the
    three tile rows of the blend, so one band is empty; four VAE tiles per rank).  At most 4 ranks: with this process they are the
    processes that have the shared GPU open at once, and a GPU machine allows no more than 6.  bench.py's own `debug_check` compares
    rank 0's ASSEMBLED image with the plain single-rank decode of the same latent: the sequence-parallel estimator sums its statistics
    in another order, so the bound is 1e-4 of the image range (observed ~2e-5), not bit equality.  (Until round 4 this flow was only ever
    run by hand: profiles/r3b.)"""
    import json
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1", "--master-port", str(port),
           os.path.join(root, "bench.py"), "--gpus", str(world), "--steps", "1", "--warmup", "0", "--latent", "256", "--vae-tile", "64", "--evals", "2",
           "--debug-single-device", "--no-cpu-baseline", "--no-profile-pass", "--no-f32-pass", "--no-whole-tile-pass", "--no-oracle-pass"]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, timeout=900, cwd=root)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert r.returncode == 0 and lines, r.stdout[-3000:]
    d = json.loads(lines[-1])
    assert d["n_gpus"] == world and d["debug_check"] is not None, d
    assert d["debug_check"]["image_shape"] == [1, 3, 2048, 2048]
    assert d["debug_check"]["assembled_image_rel_err_vs_single_rank"] < 1e-4, d["debug_check"]


_SMALL = ["--steps", "1", "--warmup", "0", "--latent", "256", "--vae-tile", "64", "--evals", "2", "--no-cpu-baseline", "--no-profile-pass", "--no-f32-pass",
          "--no-whole-tile-pass", "--no-oracle-pass", "--no-stress-pass", "--no-companions"]


def _bench_line(argv, timeout=900):
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MDTILE_BENCH_LAUNCHER")}
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env, timeout=timeout, cwd=root)
    lines = [l for l in r.stdout.splitlines() if l.startswith("{") and '"metric"' in l]
    assert r.returncode == 0 and len(lines) == 1, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    return json.loads(lines[0])


def test_bare_bench_command_launches_its_own_ranks(cuda):
    """`python bench.py --gpus 2 ...` with NO launcher environment (the shape of the driver's recorded N = 1 command): rc 0, exactly one JSON
    line, n_gpus = 2, a transport, and rank 0's assembled image equal to the single-rank decode.  On this one-GPU box the two ranks share
    cuda:0 (bench.py adds --debug-single-device itself when fewer GPUs than ranks are visible)."""
    d = _bench_line(["--gpus", "2"] + _SMALL)
    assert d["n_gpus"] == 2 and d["transport"] and "bench.py" in d["launcher"], d
    assert d["process_model"] == "one process per GPU" and d["devices_visible"] >= 1
    if d["devices_visible"] < 2:
        assert d["debug_check"] is not None and d["debug_check"]["assembled_image_rel_err_vs_single_rank"] < 1e-4, d["debug_check"]


@pytest.mark.parametrize("n", [2, 8])
def test_single_process_bench_form(cuda, n):
    """`python bench.py --gpus N --single-process`: mdtile.Shard(dev_ids) + ShardedBlend + VAEHook.devices in ONE process (what a webui can
    use) -- timed line with n_gpus = N, and with --full the assembled image bit-identical to the one-device sweep, the sharded blend
    equal to the one-device blend on every band's rows (one-GPU box: cuda:0 listed N times, copy transport)."""
    d = _bench_line(["--gpus", str(n), "--single-process", "--full"] + _SMALL)
    assert d["n_gpus"] == n and d["process_model"].startswith("single-process") and len(d["devices"]) == n, d
    assert d["transport"].startswith(("rccl", "copy")), d["transport"]
    chk = d["debug_check"]
    assert chk["assembled_image_bit_identical_to_one_device"] is True and chk["image_shape"] == [1, 3, 2048, 2048], chk
    assert chk["sharded_blend_max_abs_diff_vs_one_device"] < 1e-5, chk


def test_bring_up_probe_is_interruptible(plugin, cuda):
    """mdtile_shard_probe_rank: the rendezvous of ncclCommInitRank on a NON-BLOCKING communicator, polled under a deadline and aborted on it.
    (1) a one-rank probe comes up; (2) rank 0 of a TWO-rank communicator whose peer never shows up gives up on the deadline with an error --
    the calling thread comes back (a blocking ncclCommInitRank would sit in the rendezvous for ever: the case the round-3 review flagged,
    bring-up worker threads left inside RCCL); (3) a regular communicator still comes up afterwards.  The probe runs in a guarded thread so
    that a librccl that blocks anyway fails this test instead of hanging the suite."""
    import threading
    import time
    E = plugin.engine
    dev = cuda.index or 0

    def guarded(fn, limit):
        box = {}

        def work():
            torch.cuda.set_device(dev)
            try:
                box["value"] = fn()
            except BaseException as e:      # noqa: BLE001
                box["error"] = e
        t = threading.Thread(target=work, daemon=True)
        t0 = time.time()
        t.start()
        t.join(limit)
        assert not t.is_alive(), f"the probe did not return within {limit} s"
        return box, time.time() - t0

    box, _ = guarded(lambda: E.Shard.probe(1, 0, E.Shard.unique_id(), dev, timeout_s=30.0), 60.0)
    if "error" in box and "has no ncclCommInitRankConfig" in str(box["error"]):
        pytest.skip("this librccl has no non-blocking bring-up calls")
    assert "error" not in box, box.get("error")
    box, took = guarded(lambda: E.Shard.probe(2, 0, E.Shard.unique_id(), dev, timeout_s=2.0), 60.0)
    assert isinstance(box.get("error"), E.MdtileError) and "did not come up" in str(box["error"]), box
    assert took < 30.0
    sh = E.Shard(nranks=1, rank=0, uid=E.Shard.unique_id(), device=dev)      # the process can still build communicators
    assert sh.nranks == 1
    sh.destroy()
