"""A/B of inpaint tile skipping under the jittered grid (csrc/lattice.hip: k_lattice_blend<..., SPARSE>, k_lattice_gather<T, SPARSE>,
k_lattice_activity, k_lattice_slots) against the calls of before, the protocol of probes/lattice_regions_ab.py: one process, COLD
(rotating buffer sets larger than the 256 MiB Infinity Cache), 20 back-to-back evaluations per HIP-event pair, median of 7 rounds, the arms
ALTERNATING inside every round in an order rotated per round -- at latent 1024^2, tile 128 / overlap 0 and 128 / 8, fp32 and fp16, N = 2, C = 4,
MultiDiffusion and Mixture of Diffusers, at rest and at the shift (5, 3).  One evaluation = the gather + the blend:
    (a) rest / (5, 3)   mdtile_gather_all_lattice + mdtile_blend_lattice: every tile.  The baseline; its kernels are the parent commit's (the device
                        code of lattice.hip's earlier kernels was compared with the parent's and is identical)
    (b) rest / (5, 3)   mdtile_gather_all_lattice_sparse + mdtile_blend_lattice_sparse with ALL tiles active: what the new kernels cost a step that
                        never takes them (a step with Ta == T runs (a))
    (c) rest / (5, 3)   the same pair with 9 tiles active (a 3 x 3 block in the middle of the canvas), fill = the input
    fixed grid 9        beside (c): mdtile_gather_all + mdtile_blend_sparse on the sparse plan of the same 3 x 3 block of the FIXED grid
    copy of (a) / (c)   mdtile_stream_copy of half the bytes the pair moves (a copy reads and writes its size): the floor
(b) is checked first against (a), bitwise.  Then the per-step decision, timed on the host because it ends in a device-to-host copy:
    mdtile_lattice_activity + the flags to the host   against   mdtile_tile_activity + the flags to the host
    python probes/lattice_sparse_ab.py            (on the GPU box; the shipping library)"""
import ctypes
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C, BS = 2, 4, 8
N_CALLS, ROUNDS = 20, 7


def timed_alternating(arms):
    """arms: name -> list of callables (one per buffer set).  Every round times each arm once, in an order rotated from round to round
    -> name -> (median us, best us)."""
    for calls in arms.values():
        for c in calls[:3]:
            c()
    ts = {name: [] for name in arms}
    names = list(arms)
    for r in range(ROUNDS):
        for name in names[r % len(names):] + names[:r % len(names)]:
            calls = arms[name]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(N_CALLS):
                calls[i % len(calls)]()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e) / N_CALLS * 1e3)
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in ts.items()}


def middle_block(cols, rows):
    """Flags of a 3 x 3 block of tiles in the middle of a cols x rows grid."""
    c0, r0 = cols // 2 - 1, rows // 2 - 1
    return [1 if c0 <= t % cols < c0 + 3 and r0 <= t // cols < r0 + 3 else 0 for t in range(cols * rows)]


def ranks(flags):
    out, n = [], 0
    for a in flags:
        out.append(n if a else -1)
        n += 1 if a else 0
    return out


class Evaluation:
    """One evaluation on fixed buffers, its C arguments built once.  kind: "full" (the lattice's calls), "sparse" (the subset's calls, fill = x),
    "fixed" (mdtile_gather_all + mdtile_blend_sparse on a sparse plan)."""

    def __init__(self, kind, grid, method, x, tiles, out, maps):
        L_ = E.lib()
        dt, st, nb, xp = E.dtype_code(x.dtype), E._stream(), len(tiles), x.data_ptr()
        m = maps if kind == "fixed" else dict(tile_w=maps.get("tile_w"))
        _, self.a, self.ptrs = E._blend_operands(grid, method, tiles, N, C, x.dtype, x.dtype, x.device, out, m.get("weights"), m.get("tile_w"), m.get("rescale"))
        a, ptrs = ctypes.byref(self.a), self.ptrs
        self.keep = (grid, x, tiles, out, maps)
        if kind == "fixed":
            h = grid.handle
            self.steps = [lambda: L_.mdtile_gather_all(h, dt, N, C, xp, ptrs, nb, st), lambda: L_.mdtile_blend_sparse(h, a, ptrs, nb, xp, st)]
        elif kind == "full":
            ref = grid.ref
            self.steps = [lambda: L_.mdtile_gather_all_lattice(ref, dt, N, C, xp, ptrs, nb, st), lambda: L_.mdtile_blend_lattice(ref, a, ptrs, nb, st)]
        else:
            ref = grid.ref
            self.steps = [lambda: L_.mdtile_gather_all_lattice_sparse(ref, dt, N, C, xp, ptrs, nb, st),
                          lambda: L_.mdtile_blend_lattice_sparse(ref, a, ptrs, nb, xp, st)]
        for s_ in self.steps:
            assert s_() == 0, L_.mdtile_last_error()

    def __call__(self):
        for s_ in self.steps:
            s_()


def run(W, H, tile, ov, dtype):
    plain = E.Plan(W, H, tile, tile, ov, BS)
    stride = plain.tile_w - plain.overlap
    lattices = {"rest": E.Lattice(W, H, tile, tile, ov, BS, stride, stride), "(5, 3)": E.Lattice(W, H, tile, tile, ov, BS, 5, 3)}
    es = 4 if dtype == torch.float32 else 2
    tile_w = E.gaussian_weights(plain.tile_w, plain.tile_h, dev)
    most = max(l.num_tiles for l in lattices.values())
    canvas = es * N * C * H * W
    tile_bytes = es * N * C * plain.tile_h * plain.tile_w
    moved = 3 * most * tile_bytes + canvas                 # gather: read + write the tiles; blend: read them, write the canvas
    moved9 = 3 * 9 * tile_bytes + 2 * canvas               # ... of 9 tiles, and fill read wherever the canvas is not live
    sets = max(3, int(700e6 // moved) + 1)
    print(f"\nlatent {W} x {H}, tile {plain.tile_w} / overlap {plain.overlap}, {str(dtype).split('.')[-1]}: "
          + ", ".join(f"{k} {l.num_tiles} tiles in {l.num_batches} batches" for k, l in lattices.items())
          + f" (plain plan: {plain.num_tiles}); N = {N}, C = {C}; {moved / 1e6:.0f} MB per full pair, {moved9 / 1e6:.0f} MB with 9 tiles, {sets} buffer sets",
          flush=True)
    xs = [torch.randn(N, C, H, W, device=dev).to(dtype) for _ in range(sets)]
    outs = [torch.empty(N, C, H, W, dtype=dtype, device=dev) for _ in range(sets)]

    def tile_bufs(grid):
        return [[torch.empty(len(b) * N, C, plain.tile_h, plain.tile_w, dtype=dtype, device=dev) for b in grid.batches] for _ in range(sets)]

    def subset(lat, flags):
        return E.LatticeSubset(lat, flags, BS, torch.tensor(ranks(flags), dtype=torch.int32, device=dev))

    subs_all = {k: subset(l, [1] * l.num_tiles) for k, l in lattices.items()}
    subs_9 = {k: subset(l, middle_block(l.cols, l.rows)) for k, l in lattices.items()}
    fixed9 = plain.subset(middle_block(plain.cols, plain.rows), BS)
    bufs = {k: tile_bufs(l) for k, l in lattices.items()}
    bufs9 = {k: tile_bufs(s) for k, s in subs_9.items()}
    fixed_bufs = tile_bufs(fixed9)
    copies = {n_: [(torch.empty(n_ // 2 // 16 * 16, dtype=torch.uint8, device=dev), torch.empty(n_ // 2 // 16 * 16, dtype=torch.uint8, device=dev))
                   for _ in range(sets)] for n_ in (moved, moved9)}
    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        md = method == E.METHOD_MD
        weights = torch.zeros(H, W, device=dev)
        E.weight_map_add_grid(plain, None if md else tile_w, weights)
        lat_maps = dict(tile_w=None if md else tile_w)
        plain_maps = dict(weights=weights) if md else dict(tile_w=tile_w, rescale=E.reciprocal(weights))

        # correctness first: (b) == (a), bitwise, at rest and shifted
        bits = torch.int32 if dtype == torch.float32 else torch.int16
        for key, lat in lattices.items():
            Evaluation("full", lat, method, xs[0], bufs[key][0], outs[0], lat_maps)()
            want = outs[0].clone()
            outs[0].fill_(float("nan"))
            Evaluation("sparse", subs_all[key], method, xs[0], bufs[key][0], outs[0], lat_maps)()
            print(f"  {name} {key}: sparse pair with all tiles active == gather_all_lattice + blend_lattice: {torch.equal(outs[0].view(bits), want.view(bits))}",
                  flush=True)

        arms = {}
        for key, lat in lattices.items():
            arms[f"(a) {key}: gather_all_lattice + blend_lattice"] = [Evaluation("full", lat, method, xs[i], bufs[key][i], outs[i], lat_maps) for i in range(sets)]
            arms[f"(b) {key}: sparse pair, all {lat.num_tiles} tiles active"] = [Evaluation("sparse", subs_all[key], method, xs[i], bufs[key][i], outs[i], lat_maps)
                                                                                 for i in range(sets)]
            arms[f"(c) {key}: sparse pair, 9 of {lat.num_tiles} tiles active"] = [Evaluation("sparse", subs_9[key], method, xs[i], bufs9[key][i], outs[i], lat_maps)
                                                                                  for i in range(sets)]
        arms[f"fixed grid: gather_all + blend_sparse, 9 of {plain.num_tiles}"] = [Evaluation("fixed", fixed9, method, xs[i], fixed_bufs[i], outs[i], plain_maps)
                                                                                  for i in range(sets)]
        arms["copy of (a)'s bytes"] = [E.StreamCopyCall(s_, d_) for s_, d_ in copies[moved]]
        arms["copy of (c)'s bytes"] = [E.StreamCopyCall(s_, d_) for s_, d_ in copies[moved9]]
        res = timed_alternating(arms)
        for arm, (med, best) in res.items():
            key = arm.split(":")[0][4:]
            ref = res.get(f"(a) {key}: gather_all_lattice + blend_lattice", res["(a) rest: gather_all_lattice + blend_lattice"])[0]
            print(f"  {name} {arm:64s} {med:8.2f} us (best {best:7.2f})  x{med / ref:5.3f} of (a)", flush=True)


def decision(W, H, tile, ov):
    """The per-step decision, host-timed (it ends in a copy to the host): median of 200."""
    plain = E.Plan(W, H, tile, tile, ov, BS)
    lat = E.Lattice(W, H, tile, tile, ov, BS, 5, 3)
    mask = torch.zeros(1, H, W, device=dev)
    mask[:, H // 2 - 40:H // 2 + 40, W // 2 - 40:W // 2 + 40] = 1.0

    def med(fn):
        for _ in range(20):
            fn()
        ts = []
        for _ in range(200):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e6)
        return sorted(ts)[len(ts) // 2]

    a = med(lambda: E.lattice_activity(lat, mask))
    b = med(lambda: E.tile_activity(plain, mask))
    flags, _ = E.lattice_activity(lat, mask)
    print(f"\nper-step decision at {W} x {H}, tile {tile} / {ov}: lattice_activity + flags to the host ({sum(flags)} of {lat.num_tiles} active) {a:7.1f} us; "
          f"tile_activity + flags to the host ({plain.num_tiles} tiles) {b:7.1f} us", flush=True)


def main():
    for (tile, ov) in ((128, 0), (128, 8)):
        for dtype in (torch.float32, torch.float16):
            run(1024, 1024, tile, ov, dtype)
            torch.cuda.empty_cache()
        decision(1024, 1024, tile, ov)


if __name__ == "__main__":
    main()
