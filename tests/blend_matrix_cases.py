"""Case table of the blend-kernel matrix (a plain module, no fixtures): which geometry, dtype, method, plane count, batch form and rank
mode is meant to reach WHICH blend kernel.  Every label here is written down by hand from the dispatch rules in csrc/blend.hip;
tests/test_blend_dispatch.py (no GPU) asks the library's own dispatch query (mdtile_blend_dispatch -- the function the launcher calls)
whether each case really lands where its label says, and whether the labelled cases together reach every instantiation that ships.
tests/test_gpu_blend_matrix.py then runs the cases on the GPU, bitwise against the oracle.

k_blend_lds instantiations: 3 dtypes x 2 methods x LPP {4, 2, 1} x packed / unpacked = 36 (tile range, partial sums and row bands are
runtime flags of the same code).  k_blend: per dtype the 16-byte vector path (`vec`) and the per-element path (`elem`)."""
from collections import namedtuple

# name -> (W, H, tile_w, tile_h, overlap, tile_bs), latent pixels
GEOMETRIES = {
    "odd200": (200, 136, 96, 96, 48, 4),        # origins 0, 34, 69, 104: 3 covering columns, 2 covering rows
    "odd3rows": (200, 184, 96, 96, 48, 4),      # the same columns over three tile rows (origins 0, 44, 88): a band per rank for 3 ranks
    "odd203": (203, 141, 96, 96, 48, 4),        # the same with an odd canvas width: odd row pitch, ragged last quad
    "stock512": (512, 512, 96, 96, 48, 4),      # upstream's stock grid (origins 0, 46, 92, ...), 3 x 3 covering tiles
    "b441": (1024, 1024, 96, 96, 48, 1),        # 441 tile batches > 320 kernel-argument pointers: packed; 21 tile columns per strip
    "lanes5": (170, 130, 40, 40, 13, 4),        # 80-byte half rows: 5 DMA lanes
    "lanes64": (1000, 300, 256, 128, 16, 4),    # fp32 rows of exactly 1 KiB: all 64 DMA lanes, the limit
    "lanes33": (1000, 300, 264, 128, 16, 4),    # fp32 rows > 1 KiB -> k_blend; half rows 528 B -> LDS with 33 lanes
    "row200B": (230, 150, 100, 72, 30, 4),      # fp32 rows 400 B -> LDS; half rows 200 B (no 16-byte records) -> k_blend on odd origins 65, 130
    "onerow": (333, 96, 96, 96, 48, 4),         # a single tile row
    "mult4": (128, 96, 48, 48, 24, 4),          # origins 0, 20, 40, 60, 80: every quad whole inside its tiles -> k_blend, vector path only
}

DTYPES = ("f32", "f16", "bf16")
METHODS = ("md", "mod")

# kernel by (geometry, dtype): "lds" = k_blend_lds, "plain" = k_blend; and for k_blend the load paths its quads take
_KERNEL = {name: dict(f32="lds", f16="lds", bf16="lds") for name in GEOMETRIES}
_KERNEL["lanes33"]["f32"] = "plain"
_KERNEL["row200B"]["f16"] = _KERNEL["row200B"]["bf16"] = "plain"
_KERNEL["mult4"] = dict(f32="plain", f16="plain", bf16="plain")
_PATHS = {"lanes33": ("vec", "elem"), "row200B": ("vec", "elem"), "mult4": ("vec",)}

# planes per block of k_blend_lds: the largest of 4, 2, 1 that divides N * C and keeps the stage under 64 KB
_LPP = {(2, 4): 4, (1, 4): 4, (1, 2): 2, (1, 3): 1}
_LPP_BY_STAGE = {("b441", "f32", 1, 4): 2}     # 3 rows x 21 columns x (384 + 32) B x 4 planes = 104832 B > 64 KB -> 2 planes

# mode: "full" | "rows" (row_range) | "partial" (partial sums of a tile range) | "band" (tile range + partial + row range: one rank's launch)
Case = namedtuple("Case", "id geom dtype method N C packed mode aligned kernel lpp paths")


def _case(geom, dtype, method, N, C, packed=False, mode="full", aligned=True, tag=""):
    kernel = _KERNEL[geom][dtype] if aligned else "plain"            # misaligned batch tensors: always k_blend
    lpp = _LPP_BY_STAGE.get((geom, dtype, N, C), _LPP[(N, C)]) if kernel == "lds" else None
    paths = None if kernel == "lds" else _PATHS.get(geom, ("vec", "elem"))
    cid = "-".join([tag or "case", geom, dtype, method, f"n{N}c{C}", "packed" if packed else "ptrs", mode] + ([] if aligned else ["misaligned"]))
    return Case(cid, geom, dtype, method, N, C, packed, mode, aligned, kernel, lpp, paths)


# ---- delegate path: one model evaluation through MultiDiffusion / MixtureOfDiffusers, every geometry of the table
DELEGATE_CASES = [_case(g, dt, m, 1 if g == "b441" else 2, 4, packed=(g == "b441"), tag="delegate")
                  for g in GEOMETRIES for dt in DTYPES for m in METHODS]

# ---- engine path: (geometry, dtype, method, N, C) groups; each runs packed and unpacked, full / row band / partial sums of tile ranges
ENGINE_GEOMETRIES = ("odd200", "odd203")
ENGINE_PLANES = ((2, 4), (1, 2), (1, 3))        # -> LPP 4, 2, 1
ENGINE_GROUPS = [(g, dt, m, N, C) for g in ENGINE_GEOMETRIES for dt in DTYPES for m in METHODS for (N, C) in ENGINE_PLANES]
ENGINE_CASES = [_case(g, dt, m, N, C, packed=pk, mode=mode, tag="engine")
                for (g, dt, m, N, C) in ENGINE_GROUPS for pk in (False, True) for mode in ("full", "rows", "partial", "band")]

# ---- batch tensors that are views offset by one element: not 16-byte aligned -> k_blend, same bits
MISALIGNED_CASES = [_case("odd200", dt, m, 2, 4, aligned=False, tag="misaligned") for dt in DTYPES for m in METHODS]

# ---- special values: an LDS grid and a k_blend grid, fp32 and fp16 (3-fold overlaps on odd200: columns 69..95 are covered by 3 tiles)
SPECIAL_CASES = [_case(g, dt, m, 1, 4, tag="special") for g in ("odd200", "lanes33", "row200B") for dt in ("f32", "f16") for m in METHODS]

# ---- sharded: every band's launch (tile range + partial + row range, packed) on an odd-origin grid
SHARD_GEOMETRIES = ("odd200", "odd3rows")
SHARD_CASES = [_case(g, dt, m, 2, 4, packed=True, mode="band", tag="shard") for g in SHARD_GEOMETRIES for dt in ("f32", "f16") for m in METHODS]

CASES = DELEGATE_CASES + ENGINE_CASES + MISALIGNED_CASES + SPECIAL_CASES + SHARD_CASES


def tile_ranges(plan):
    """The two splits of the tile list the partial-sum cases use: at a tile-row boundary and at a tile index in the middle of a tile row."""
    T, cols = plan.num_tiles, plan.cols
    at_row = max(1, plan.rows // 2) * cols if plan.rows > 1 else max(1, cols // 2)
    mid_row = min(T - 1, cols + cols // 2) if plan.rows > 1 else max(1, cols // 2 + 1)
    return [((0, at_row), (at_row, T)), ((0, mid_row), (mid_row, T))]


def row_band(plan):
    """A canvas row band of about a third of the canvas: on the two-row grids of the engine cases it starts and ends inside the overlap."""
    return (plan.h // 3, (2 * plan.h) // 3 + 1)
