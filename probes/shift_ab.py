"""A/B of the shifted wrap-around grid (csrc/wrap.hip: k_wrap_gather<T, SHIFT>, k_walk_blend<..., SHIFT>) against the unshifted pair
on the same plan, the protocol of probes/wrap_ab.py and probes/sparse_blend_ab.py: one process, COLD (rotating buffer sets larger than the
256 MiB Infinity Cache), 20 back-to-back calls per HIP-event pair, median of 7 rounds, the arms ALTERNATING inside every round -- at latent
1024^2 closed in both axes, tile 128 / overlap 8 and 128 / 0, fp32, N = 2, C = 4, MultiDiffusion and Mixture of Diffusers:
    plain          mdtile_gather_all + mdtile_blend.  Their kernels are the parent commit's: the instruction streams of every k_wrap_gather<*> and
                   every k_walk_blend<*> that is not shifted were compared with the parent's after cross-compiling both, and are identical
    shift (sx, 0)  mdtile_gather_all_shift + mdtile_blend_shift for sx in {0, 4, 1, W - 2}: aligned without a move, aligned, odd (every store of
                   four elements off its 16-byte boundary), and the last quad of every row cut by the seam; and (1, 3), rows moved as well
    copy           mdtile_stream_copy of a pair's bytes (canvas read + tiles written + tiles read + canvas written): the floor
The shifted pair is checked first against torch.roll around the plain pair, bitwise.
    python probes/shift_ab.py            (on the GPU box; the shipping library)"""
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
    """One gather + blend pair on fixed buffers with its C arguments built once; shift None: mdtile_gather_all + mdtile_blend."""

    def __init__(self, plan, method, x, tiles, out, maps, shift=None):
        L_ = E.lib()
        self.keep = (plan, x, tiles, out, maps)
        _, self.a, self.ptrs = E._blend_operands(plan, method, tiles, N, C, x.dtype, x.dtype, x.device, out, maps.get("weights"), maps.get("tile_w"),
                                                 maps.get("rescale"))
        h, dt, nb, xp = plan.handle, E.dtype_code(x.dtype), len(tiles), x.data_ptr()
        a, ptrs, st = ctypes.byref(self.a), self.ptrs, E._stream()
        if shift is None:
            self.gather = lambda: L_.mdtile_gather_all(h, dt, N, C, xp, ptrs, nb, st)
            self.blend = lambda: L_.mdtile_blend(h, a, ptrs, nb, None, 0, st)
        else:
            sx, sy = shift
            self.gather = lambda: L_.mdtile_gather_all_shift(h, dt, N, C, xp, ptrs, nb, sx, sy, st)
            self.blend = lambda: L_.mdtile_blend_shift(h, a, ptrs, nb, sx, sy, st)
        assert self.gather() == 0 and self.blend() == 0, L_.mdtile_last_error()


def run(ov):
    plan = E.Plan(L, L, TILE, TILE, ov, BS, wrap_x=True, wrap_y=True)
    T = plan.num_tiles
    weights = torch.zeros(L, L, device=dev)
    E.weight_map_add_grid(plan, None, weights)
    tile_w = E.gaussian_weights(plan.tile_w, plan.tile_h, dev)
    gsum = torch.zeros(L, L, device=dev)
    E.weight_map_add_grid(plan, tile_w, gsum)
    maps = {E.METHOD_MD: dict(weights=weights), E.METHOD_MOD: dict(tile_w=tile_w, rescale=E.reciprocal(gsum))}
    canvas = 4 * N * C * L * L
    tile_bytes = 4 * N * C * plan.tile_h * plan.tile_w
    moved = 2 * T * tile_bytes + 2 * canvas
    sets = max(3, int(700e6 // moved) + 1)
    print(f"\nlatent {L}^2 torus, tile {plan.tile_w} / overlap {plan.overlap}: {T} tiles in {plan.num_batches} batches; N = {N}, C = {C}, fp32; "
          f"{moved / 1e6:.0f} MB per gather + blend pair, {sets} buffer sets", flush=True)
    xs = [torch.randn(N, C, L, L, device=dev) for _ in range(sets)]
    outs = [torch.empty(N, C, L, L, device=dev) for _ in range(sets)]
    bufs = [[torch.empty(len(b) * N, C, plan.tile_h, plan.tile_w, device=dev) for b in plan.batches] for _ in range(sets)]
    shifts = [(0, 0), (4, 0), (1, 0), (L - 2, 0), (1, 3)]

    # correctness first: the roll identity on the device, bitwise
    for method, name in ((E.METHOD_MD, "MultiDiffusion"), (E.METHOD_MOD, "Mixture of Diffusers")):
        for (sx, sy) in shifts:
            tiles = E.gather_all_shift(plan, xs[0], sx, sy)
            same_tiles = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                             for a, b in zip(tiles, E.gather_all(plan, torch.roll(xs[0], (-sy, -sx), (-2, -1)).contiguous())))
            got = E.blend_shift(plan, method, tiles, N, C, sx=sx, sy=sy, **maps[method])
            want = torch.roll(E.blend(plan, method, tiles, N, C, **maps[method]), (sy, sx), (-2, -1))
            print(f"  {name} ({sx}, {sy}): gather == gather(roll) {same_tiles}, blend_shift == roll(blend) "
                  f"{torch.equal(got.view(torch.int32), want.view(torch.int32))}", flush=True)

    half = moved // 2 // 16 * 16
    copies = [E.StreamCopyCall(torch.randn(half // 4, device=dev), torch.empty(half // 4, device=dev)) for _ in range(sets)]
    for method, name in ((E.METHOD_MD, "md "), (E.METHOD_MOD, "mod")):
        # every arm is marshalled ONCE (argument struct, pointer arrays) and a timed call is the two C calls alone: the host work per call is the
        # same on either side and far below the kernels' time
        plain_calls = [Prepared(plan, method, xs[i], bufs[i], outs[i], maps[method]) for i in range(sets)]
        shift_calls = {s_: [Prepared(plan, method, xs[i], bufs[i], outs[i], maps[method], s_) for i in range(sets)] for s_ in shifts}

        def plain(i):
            plain_calls[i].gather()
            plain_calls[i].blend()

        def shifted(i, sx, sy):
            shift_calls[(sx, sy)][i].gather()
            shift_calls[(sx, sy)][i].blend()

        arms = {"plain: gather_all + blend": [(lambda i=i: plain(i)) for i in range(sets)]}
        for (sx, sy) in shifts:
            arms[f"shift ({sx}, {sy}): gather_all_shift + blend_shift"] = [(lambda i=i, sx=sx, sy=sy: shifted(i, sx, sy)) for i in range(sets)]
        arms[f"stream copy {half / 1e6:.0f} MB -> {half / 1e6:.0f} MB (the pair's bytes)"] = copies
        res = timed_alternating(arms)
        base = res["plain: gather_all + blend"][0]
        for arm, (med, best) in res.items():
            print(f"  {name} {arm:58s} {med:8.2f} us (best {best:7.2f})  {moved / med * 1e-3:7.0f} GB/s  x{med / base:5.3f} of plain", flush=True)

        # the blend alone, on tiles gathered once
        for i in range(sets):
            E.gather_all(plan, xs[i], out=bufs[i])
        arms = {"plain: blend alone": [c.blend for c in plain_calls]}
        for (sx, sy) in shifts:
            arms[f"shift ({sx}, {sy}): blend_shift alone"] = [c.blend for c in shift_calls[(sx, sy)]]
        res = timed_alternating(arms)
        base = res["plain: blend alone"][0]
        for arm, (med, best) in res.items():
            print(f"  {name} {arm:58s} {med:8.2f} us (best {best:7.2f})  {(moved // 2) / med * 1e-3:7.0f} GB/s  x{med / base:5.3f} of plain", flush=True)


def main():
    for ov in (8, 0):
        run(ov)


if __name__ == "__main__":
    main()
