"""A/B of Tiled VAE tile skipping (csrc/vae_skip.hip), the protocol of probes/seam_blend_ab.py: one process, COLD (rotating
buffer sets larger than the 256 MiB Infinity Cache), back-to-back launches per HIP-event pair, median of 7 rounds; decodes by wall clock,
alternating arms in one process, 3 per arm.
    activity   mask_activity_u8 on an 8192^2 mask over the 16 out boxes of tile 256 -- the kernel alone (events), and the whole decision as
               the hook makes it (upload of the mask's bytes, upload of the boxes, launch, flag copy; wall clock) -- against mdtile_stream_copy
               of the mask's bytes and against the same decision in numpy on the host
    assembly   mdtile_vae_assemble_sparse with 16, 4 and 1 of the 16 tiles present (the rest filled from a byte image, and with NULL) against
               mdtile_vae_assemble on the same table, against the parent commit's mdtile_vae_assemble when --parent-lib names a library built
               from it, and against mdtile_stream_copy of the result's bytes
    decode     the whole 8K fast decode (SD-topology decoder, default-init weights) with 1, 2 and 4 of 16 tiles active at tile 256 and a
               face-sized mask at tile 64, against the full decode (option off: the parent commit's path, its assembly kernel recompiled)
    python probes/vae_skip_ab.py [--parent-lib PATH] [--no-decode]            (on the GPU box; the shipping library)"""
import ctypes
import os
import sys
import time
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C, L, TS = 1, 3, 1024, 256


def timed(calls, n=20, rounds=7):
    for c in calls[:3]:
        c()
    ts = []
    for _ in range(rounds):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for i in range(n):
            calls[i % len(calls)]()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / n * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def wall(call, n=7):
    call()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1]


def report(name, us, nbytes):
    med, best, worst = us
    print(f"  {name:58s} {med:9.2f} us (best {best:8.2f}, worst {worst:8.2f})  {nbytes / med * 1e-3:7.0f} GB/s", flush=True)


def activity():
    RH = RW = 8 * L
    _, outs = E.vae_split_tiles(L, L, TS, True)
    nbytes = RH * RW
    sets = max(3, int(700e6 // nbytes) + 1)
    print(f"activity: mask {RH} x {RW} ({nbytes / 1e6:.0f} MB), {len(outs)} boxes, {sets} buffer sets")
    host = np.zeros((RH, RW), np.uint8)
    host[4000:4400, 4000:4300] = 255                     # a face: one tile of 16
    masks = [torch.from_numpy(host).to(dev) for _ in range(sets)]
    d_boxes = torch.tensor(outs, dtype=torch.int32, device=dev)
    flags = torch.empty(len(outs), dtype=torch.int32, device=dev)
    L_ = E.lib()
    s = torch.cuda.current_stream().cuda_stream

    def kernel(m):
        rc = L_.mdtile_mask_activity_u8(m.data_ptr(), RH, RW, d_boxes.data_ptr(), len(outs), flags.data_ptr(), s)
        assert rc == 0
    got = E.mask_activity_u8(masks[0], outs)
    want = [int(host[b[2]:b[3], b[0]:b[1]].any()) for b in outs]
    print(f"  flags == numpy: {got == want} ({sum(got)} of {len(got)} active)")
    # (the C call copies the boxes to the host for its check and waits for the stream: each call is one round trip)
    report("mdtile_mask_activity_u8, mask on the device", wall(lambda: [kernel(m) for m in masks][0], n=7), nbytes * sets)
    cps = [E.StreamCopyCall(torch.empty(nbytes // 4, device=dev), torch.empty(nbytes // 4, device=dev)) for _ in range(sets)]
    report(f"stream copy {nbytes / 1e6:.0f} MB -> {nbytes / 1e6:.0f} MB", timed(cps), 2 * nbytes)
    report("the hook's decision: upload + boxes + launch + flags", wall(lambda: E.mask_activity_u8(torch.from_numpy(host).to(dev), outs)), nbytes)
    report("numpy on the host: mask[y1:y2, x1:x2].any() per box", wall(lambda: [host[b[2]:b[3], b[0]:b[1]].any() for b in outs]), nbytes)
    full = np.zeros((RH, RW), np.uint8)                  # the worst case of the early exit: nothing set, every byte read
    report("numpy on the host, empty mask", wall(lambda: [full[b[2]:b[3], b[0]:b[1]].any() for b in outs]), nbytes)
    zero = [torch.zeros(RH, RW, dtype=torch.uint8, device=dev) for _ in range(sets)]
    report("mdtile_mask_activity_u8, empty mask on the device", wall(lambda: [kernel(m) for m in zero][0], n=7), nbytes * sets)


def parent_assemble(path):
    """mdtile_vae_assemble of a library built from the parent commit, as a call on the binding's tile tables."""
    lib = ctypes.CDLL(path)
    fn = lib.mdtile_vae_assemble
    fn.restype, fn.argtypes = E._SIGNATURES["mdtile_vae_assemble"]

    def call(tiles, result):
        n, c, RH, RW = result.shape
        table = (E._VaeTile * len(tiles))()
        for k, (t, ib, ob) in enumerate(tiles):
            table[k] = E._VaeTile(t.data_ptr(), t.shape[2], t.shape[3], (ctypes.c_int * 4)(*ib), (ctypes.c_int * 4)(*ob))
        rc = fn(table, len(tiles), n, c, 1, result.data_ptr(), RH, RW, torch.cuda.current_stream().cuda_stream)
        assert rc == 0
    return call


def assembly(parent_lib):
    ins, outs = E.vae_split_tiles(L, L, TS, True)
    assert len(ins) == 16
    RH = RW = L * 8
    nbytes = 2 * 4 * N * C * RH * RW
    sets = max(3, int(700e6 // nbytes) + 1)
    print(f"8K decode assembly: {len(ins)} tiles of up to {max((i[1] - i[0]) * 8 for i in ins)} px, result {N}x{C}x{RH}x{RW} "
          f"({nbytes / 2e6:.0f} MB written), {sets} buffer sets")
    bufs = [([(torch.randn(N, C, (ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8, device=dev), ib, ob) for ib, ob in zip(ins, outs)],
             torch.empty(N, C, RH, RW, device=dev)) for _ in range(sets)]
    fill = torch.randint(0, 256, (RH, RW, C), dtype=torch.uint8, device=dev)
    tiles, out = bufs[0]
    plain = torch.empty_like(out)
    E.vae_assemble(tiles, plain, True)
    E.vae_assemble_sparse(tiles, [], fill, out)
    torch.cuda.synchronize()
    print(f"  16 of 16 present == mdtile_vae_assemble, bitwise: {torch.equal(out.view(torch.int32), plain.view(torch.int32))}")
    report("plain (mdtile_vae_assemble, this commit)", timed([(lambda t=t, o=o: E.vae_assemble(t, o, True)) for t, o in bufs]), nbytes)
    if parent_lib:
        pa = parent_assemble(parent_lib)
        pa(tiles, out)
        torch.cuda.synchronize()
        print(f"  parent's mdtile_vae_assemble == this commit's, bitwise: {torch.equal(out.view(torch.int32), plain.view(torch.int32))}")
        report("plain (mdtile_vae_assemble, parent commit)", timed([(lambda t=t, o=o: pa(t, o)) for t, o in bufs]), nbytes)
        report("plain (mdtile_vae_assemble, this commit) again", timed([(lambda t=t, o=o: E.vae_assemble(t, o, True)) for t, o in bufs]), nbytes)
    for present in (16, 4, 1):
        keep = list(range(16))[:present] if present != 4 else [5, 6, 9, 10]
        boxes = [outs[i] for i in range(16) if i not in keep]
        written = 4 * N * C * RH * RW
        read_tiles = sum(4 * N * C * (outs[i][1] - outs[i][0]) * (outs[i][3] - outs[i][2]) for i in keep)
        for f, name in ((fill, "byte fill"), (None, "NULL")):
            read_fill = 0 if f is None else sum(C * (b[1] - b[0]) * (b[3] - b[2]) for b in boxes)
            report(f"sparse, {present:2d} of 16 present, {name}",
                   timed([(lambda t=t, o=o: E.vae_assemble_sparse([t[i] for i in keep], boxes, f, o)) for t, o in bufs]), written + read_tiles + read_fill)
    half = nbytes // 2
    cps = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(sets)]
    report(f"stream copy {half / 1e6:.0f} MB -> {half / 1e6:.0f} MB", timed(cps), nbytes)


def decode():
    from PIL import Image
    from hostsim import stub_host as sh, ldm_decoder as ld
    sh.install("cuda:0")
    sh.set_device("cuda:0")
    pl = sh.load_plugin()
    dec = ld.make_decoder(0).to(dev)
    dec.original_forward = dec.forward
    torch.manual_seed(0)
    z = torch.randn(1, 4, L, L, device=dev)
    size = (8 * L, 8 * L)
    init = Image.fromarray(np.random.RandomState(0).randint(0, 256, size=(size[1], size[0], 3)).astype(np.uint8), mode="RGB")

    def job(rects):
        m = np.zeros((size[1], size[0]), np.uint8)
        for x1, x2, y1, y2 in rects:
            m[y1:y2, x1:x2] = 255
        return SimpleNamespace(mask_for_overlay=Image.fromarray(m, mode="L"), overlay_images=[init], inpaint_full_res=False, color_corrections=None,
                               init_images=[init])

    _, outs = E.vae_split_tiles(L, L, TS, True)
    X, Y = outs[2][0], outs[8][2]                           # the border between tile columns 1 | 2 and between tile rows 1 | 2
    face = (X + 100, X + 400, Y + 100, Y + 500)             # 300 x 400 px inside tile (2, 2)
    arms = [("tile 256, full decode (option off)", TS, None),
            ("tile 256, 1 of 16 tiles active", TS, job([face])),
            ("tile 256, 2 of 16 tiles active", TS, job([(X - 150, X + 150, Y + 100, Y + 500)])),
            ("tile 256, 4 of 16 tiles active", TS, job([(X - 150, X + 150, Y - 200, Y + 200)])),
            ("tile 64, full decode (option off)", 64, None),
            ("tile 64, face-sized mask", 64, job([face]))]
    hooks = []
    for name, ts, j in arms:
        h = pl.tilevae.VAEHook(dec, ts, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
        h.inpaint_job = j
        hooks.append(h)
    times = [[] for _ in arms]
    with torch.no_grad():
        hooks[0](z)                                        # warm-up: packs the weights, fills the allocator
        for _ in range(3):
            for k, h in enumerate(hooks):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                h(z)
                torch.cuda.synchronize()
                times[k].append((time.perf_counter() - t0) * 1e3)
    for (name, ts, j), h, t in zip(arms, hooks, times):
        print(f"  8K fast decode, {name:36s}: median {sorted(t)[1]:8.1f} ms  ({', '.join(f'{v:.1f}' for v in t)})  {h.last_tiles_run} of "
              f"{len(h.last_tile_slots)} tiles run", flush=True)
    print(f"  max VRAM allocated {torch.cuda.max_memory_allocated(dev) / 2**30:.2f} GiB")


if __name__ == "__main__":
    parent = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    activity()
    torch.cuda.empty_cache()
    assembly(parent)
    torch.cuda.empty_cache()
    if "--no-decode" not in sys.argv:
        decode()
