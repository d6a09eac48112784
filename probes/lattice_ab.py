"""A/B of the jittered grid on a plain canvas (csrc/lattice.hip: k_lattice_gather, k_lattice_blend) against the plain plan's pair at
the same tile and overlap, the protocol of probes/shift_ab.py: one process, COLD (rotating buffer sets larger than the 256 MiB
Infinity Cache), 20 back-to-back calls per HIP-event pair, median of 7 rounds, the arms ALTERNATING inside every round -- gather + blend per
evaluation at latent 1024^2, tile 128 / overlap 0 and 128 / 8, fp32, N = 2, C = 4, MultiDiffusion and Mixture of Diffusers:
    plain            mdtile_gather_all + mdtile_blend on mdtile_plan_create(clamp = 1) with the plan's own maps (the parent commit's kernels)
    lattice (sx, sy) mdtile_gather_all_lattice + mdtile_blend_lattice at rest (stride, stride), at an aligned shift (4, 4) and at an odd one (5, 3);
                     a shift that is not the rest has one more tile column and row, so its pair moves more bytes: GB/s is per arm
    copy             mdtile_stream_copy of the plain pair's bytes (canvas read + tiles written + tiles read + canvas written): the floor
At rest the lattice pair is first checked against the plain pair, bitwise.  No number gates the path: what the option buys is the count of UNet
calls at a small overlap.
    python probes/lattice_ab.py            (on the GPU box; the shipping library)"""
import ctypes
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "multidiffusion-upscaler-for-automatic1111_amd"))
import mdtile as E          # noqa: E402

dev = torch.device("cuda:0")
N, C, L, TILE, BS = 2, 4, 1024, 128, 8
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
        for name in names[r % len(names):] + names[:r % len(names)]:      # a new arm leads every round: no arm always follows the same one
            calls = arms[name]
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(N_CALLS):
                calls[i % len(calls)]()
            e.record()
            torch.cuda.synchronize()
            ts[name].append(s.elapsed_time(e) / N_CALLS * 1e3)
    return {name: (sorted(t)[len(t) // 2], min(t)) for name, t in ts.items()}


class Prepared:
    """One gather + blend pair on fixed buffers with its C arguments built once; grid: a Plan (mdtile_gather_all + mdtile_blend with `maps`) or a
    Lattice (the lattice pair; only tile_w of `maps` is handed over)."""

    def __init__(self, grid, method, x, tiles, out, maps):
        L_ = E.lib()
        lattice = isinstance(grid, E.Lattice)
        self.keep = (grid, x, tiles, out, maps)
        _, self.a, self.ptrs = E._blend_operands(grid, method, tiles, N, C, x.dtype, x.dtype, x.device, out, None if lattice else maps.get("weights"),
                                                 maps.get("tile_w"), None if lattice else maps.get("rescale"))
        dt, nb, xp = E.dtype_code(x.dtype), len(tiles), x.data_ptr()
        a, ptrs, st = ctypes.byref(self.a), self.ptrs, E._stream()
        if lattice:
            ref = grid.ref
            self.gather = lambda: L_.mdtile_gather_all_lattice(ref, dt, N, C, xp, ptrs, nb, st)
            self.blend = lambda: L_.mdtile_blend_lattice(ref, a, ptrs, nb, st)
        else:
            h = grid.handle
            self.gather = lambda: L_.mdtile_gather_all(h, dt, N, C, xp, ptrs, nb, st)
            self.blend = lambda: L_.mdtile_blend(h, a, ptrs, nb, None, 0, st)
        assert self.gather() == 0 and self.blend() == 0, L_.mdtile_last_error()

    def pair(self):
        self.gather()
        self.blend()


def pair_bytes(grid):
    return 2 * grid.num_tiles * 4 * N * C * grid.tile_h * grid.tile_w + 2 * 4 * N * C * L * L


def run(ov):
    plan = E.Plan(L, L, TILE, TILE, ov, BS)
    stride = plan.tile_w - plan.overlap
    assert (L - plan.tile_w) % stride == 0 or ov != 0
    lattices = {s: E.Lattice(L, L, TILE, TILE, ov, BS, *s) for s in ((stride, stride), (4, 4), (5, 3))}
    weights = torch.zeros(L, L, device=dev)
    E.weight_map_add_grid(plan, None, weights)
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev)
    gsum = torch.zeros(L, L, device=dev)
    E.weight_map_add_grid(plan, tile_w, gsum)
    maps = {E.METHOD_MD: dict(weights=weights), E.METHOD_MOD: dict(tile_w=tile_w, rescale=E.reciprocal(gsum))}
    most = max(lat.num_tiles for lat in lattices.values())
    moved = pair_bytes(plan)
    sets = max(3, int(700e6 // moved) + 1)
    print(f"\nlatent {L}^2, tile {plan.tile_w} / overlap {plan.overlap}: plain plan {plan.num_tiles} tiles in {plan.num_batches} batches; lattice "
          + ", ".join(f"{s}: {lat.num_tiles} tiles" for s, lat in lattices.items()) + f"; N = {N}, C = {C}, fp32; {moved / 1e6:.0f} MB per plain pair, "
          f"{sets} buffer sets", flush=True)
    xs = [torch.randn(N, C, L, L, device=dev) for _ in range(sets)]
    outs = [torch.empty(N, C, L, L, device=dev) for _ in range(sets)]
    # one pool of tile memory per set, large enough for the largest lattice; every grid's batches are views into it
    pools = [torch.empty(most * N, C, plan.tile_h, plan.tile_w, device=dev) for _ in range(sets)]

    def views(pool, grid):
        return list(pool[:grid.num_tiles * N].split([len(b) * N for b in grid.batches], dim=0))

    # correctness first: where the stride divides the canvas, the lattice at rest is the plain plan, bitwise
    rest = lattices[(stride, stride)]
    if rest.bboxes == plan.bboxes:
        for method, name in ((E.METHOD_MD, "MultiDiffusion"), (E.METHOD_MOD, "Mixture of Diffusers")):
            tiles = E.gather_all_lattice(rest, xs[0])
            same_tiles = all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(tiles, E.gather_all(plan, xs[0])))
            got = E.blend_lattice(rest, method, tiles, N, C, tile_w=maps[method].get("tile_w"))
            want = E.blend(plan, method, tiles, N, C, **maps[method])
            print(f"  {name}: at rest gather == gather_all {same_tiles}, blend_lattice == blend {torch.equal(got.view(torch.int32), want.view(torch.int32))}",
                  flush=True)
    else:
        print("  the stride does not divide the canvas: the lattice at rest is not the plain plan (its last tile is pushed in), no bitwise check", flush=True)

    half = moved // 2 // 16 * 16
    copies = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(sets)]
    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        plain_calls = [Prepared(plan, method, xs[i], views(pools[i], plan), outs[i], maps[method]) for i in range(sets)]
        lat_calls = {s: [Prepared(lat, method, xs[i], views(pools[i], lat), outs[i], maps[method]) for i in range(sets)] for s, lat in lattices.items()}
        arms = {"plain: gather_all + blend": [c.pair for c in plain_calls]}
        nbytes = {"plain: gather_all + blend": moved}
        for s, lat in lattices.items():
            arm = f"lattice {s}: gather_all_lattice + blend_lattice"
            arms[arm] = [c.pair for c in lat_calls[s]]
            nbytes[arm] = pair_bytes(lat)
        copy_arm = f"stream copy {half / 1e6:.0f} MB -> {half / 1e6:.0f} MB (the plain pair's bytes)"
        arms[copy_arm] = copies
        nbytes[copy_arm] = moved
        res = timed_alternating(arms)
        base = res["plain: gather_all + blend"][0]
        for arm, (med, best) in res.items():
            print(f"  {name} {arm:62s} {med:8.2f} us (best {best:7.2f})  {nbytes[arm] / med * 1e-3:7.0f} GB/s  x{med / base:5.3f} of plain", flush=True)


def main():
    for ov in (0, 8):
        run(ov)


if __name__ == "__main__":
    main()
