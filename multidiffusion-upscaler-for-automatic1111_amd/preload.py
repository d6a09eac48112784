"""Command-line options of the extension.  A1111 calls preload(parser) for every extension before it parses the command line."""


def preload(parser):
    parser.add_argument(
        "--mdtile-devices", type=str, default=None,
        help="Tiled VAE on several GPUs of this process: comma-separated CUDA indices (a device may be listed more than once), or 'all'. "
             "The VAE's own device is always the first; the others need peer access to it. Default: the VAE's device only.")
    parser.add_argument(
        "--mdtile-precision", type=str, default=None, choices=["bf16x3", "f32", "bf16", "f16", "auto"],
        help="Matrix-core arithmetic of Tiled VAE while it is enabled: bf16x3 (split-bf16, fp32 class), f32 (exact), bf16 / f16 (one MFMA per product, "
             "the arithmetic class of a bfloat16 / float16 VAE), auto (from the VAE's dtype: float16 -> f16, bfloat16 -> bf16, else bf16x3). "
             "Default: not set, the engine's mode is left alone (bf16x3 unless the process set another).")
    parser.add_argument(
        "--mdtile-color-fix", type=str, default=None, choices=["wavelet", "adain"],
        help="Tie the colours of every Tiled Diffusion img2img result to its (upscaled) init image, on the GPU: wavelet (the result's detail over "
             "the init image's low frequencies, five dilated 3x3 levels) or adain (per-channel mean and deviation of the init image). "
             "Default: not set, results are left as decoded.")
    parser.add_argument(
        "--mdtile-wrap-x", action="store_true",
        help="Close the canvas horizontally (360-degree panoramas): Tiled Diffusion lays its tile columns on a circle, so that tiles span the seam "
             "between the right and the left edge, and Tiled VAE pads its input with the columns of the other edge instead of zeros. Region "
             "control on it needs --mdtile-wrap-regions. Default: off, the canvas is a strip with two ends.")
    parser.add_argument(
        "--mdtile-wrap-y", action="store_true",
        help="Close the canvas vertically: tile rows on a circle, tiles span the seam between the bottom and the top edge, and Tiled VAE pads its "
             "input with the rows of the other edge. With --mdtile-wrap-x the canvas is a torus (seamless textures that tile in both directions). "
             "Region control on it needs --mdtile-wrap-regions. Default: off.")
    parser.add_argument(
        "--mdtile-wrap-regions", action="store_true",
        help="Tiled Diffusion with --mdtile-wrap-x / --mdtile-wrap-y (MultiDiffusion, Mixture of Diffusers): allow region prompt control on the "
             "closed canvas. A region's rectangle is laid on the circle along every axis that wraps, so it may cross the seam (x + w past the right "
             "edge goes on at the left one); background and foreground regions, each region's own noise, ControlNet and StableSR follow it, with "
             "and without --mdtile-grid-shift. Without this option regions on a wrapped canvas are refused, as before. Ignored (one line) when no "
             "axis wraps. Not combined with Noise Inversion's renoise composite when only regions are painted, nor with the multi-GPU partial "
             "path; DemoFusion does not read it. Default: off.")
    parser.add_argument(
        "--mdtile-grid-shift", action="store_true",
        help="Tiled Diffusion with --mdtile-wrap-x / --mdtile-wrap-y (MultiDiffusion, Mixture of Diffusers): displace the whole tile grid cyclically "
             "along the wrapped axes by a new offset every sampler step (a function of the job's seed and the step), so that no tile border stays in "
             "place for two steps and small or zero overlaps become usable. Ignored on a grid that does not wrap, by Noise Inversion's own "
             "evaluations and by DemoFusion. Default: off, the grid stays where it is.")
    parser.add_argument(
        "--mdtile-grid-jitter", action="store_true",
        help="Tiled Diffusion on a plain canvas (MultiDiffusion, Mixture of Diffusers; the usual img2img upscale): lay the tile grid anew every sampler "
             "step, offset by a function of the job's seed and the step, tiles that would hang over an edge pushed inside, so that no tile border "
             "stays in place for two steps and small or zero overlaps become usable. The tile count may change by a column and a row between "
             "steps. The fixed grid runs instead (one line says why) on a canvas that wraps around (use --mdtile-grid-shift there), with region "
             "control (unless --mdtile-jitter-regions is set), when --mdtile-inpaint-skip skips tiles (unless --mdtile-jitter-inpaint-skip is set), in Noise Inversion's own evaluations, when the tile spans the canvas and beyond "
             "320 tile batches. DemoFusion does not read it. Default: off, the grid stays where it is.")
    parser.add_argument(
        "--mdtile-jitter-regions", action="store_true",
        help="Tiled Diffusion with --mdtile-grid-jitter (MultiDiffusion, Mixture of Diffusers): keep the moving grid when region prompt control "
             "is enabled. The regions stay where they were drawn, background and foreground alike; only the tile grid of the background moves, "
             "and each step's weight sum is formed from that step's grid plus the background regions. Without this option a job with regions "
             "runs the fixed grid, as before. Ignored (one line) without --mdtile-grid-jitter; with no background to draw there is no grid to "
             "move and the fixed path runs (one line). Noise Inversion's own evaluations, wrap-around canvases, --mdtile-inpaint-skip and the "
             "multi-GPU partial path stay on the fixed grid; DemoFusion does not read it. Default: off.")
    parser.add_argument(
        "--mdtile-vae-seam-blend", type=int, default=None, metavar="PX",
        help="Tiled VAE decoder: cross-fade neighbouring tiles over PX image pixels per side of a tile border (1-88; 16-32 is a sensible range), out "
             "of the padding that is otherwise decoded and thrown away, instead of pasting the tiles edge to edge. Every decoded tile is kept "
             "until the image is assembled. Default: not set, edge to edge.")
    parser.add_argument(
        "--mdtile-vae-inpaint-skip", action="store_true",
        help="img2img inpainting with Tiled VAE's fast decoder: decode only the tiles that the job's overlay mask touches and fill the others "
             "from the init image. Relies on the host pasting the original image back over the result wherever the overlay mask is zero, as "
             "the webui does for an inpaint job; a script that composites the decoded image itself (soft inpainting) is outside that premise. "
             "Not applied (one line says why) with the slow decoder, --mdtile-vae-seam-blend, a process per GPU, wrap-around, 'only masked' "
             "inpainting, the host's colour correction, a job without overlay mask or overlay images, or a mask of another size than the "
             "decoded image. Default: off, every tile is decoded.")
    parser.add_argument(
        "--mdtile-inpaint-skip", action="store_true",
        help="img2img inpainting with Tiled Diffusion (MultiDiffusion, Mixture of Diffusers): run the model only on the grid tiles that the job's "
             "latent mask touches. Relies on the host replacing the model output by the init latent wherever the mask is zero, as the webui's "
             "CFGDenoiser does; the masked area comes out bit-identical. Not applied with region control, wrap-around, Noise Inversion's own "
             "evaluations or DemoFusion. With --mdtile-grid-jitter the tiles are skipped on the fixed grid, unless --mdtile-jitter-inpaint-skip is "
             "set. Default: off, every tile runs.")
    parser.add_argument(
        "--mdtile-jitter-inpaint-skip", action="store_true",
        help="Tiled Diffusion with both --mdtile-grid-jitter and --mdtile-inpaint-skip (MultiDiffusion, Mixture of Diffusers): keep the moving "
             "grid when the inpaint mask lets tiles be skipped. Every sampler step asks which tiles of that step's grid the mask touches -- a tile "
             "counts where it contributes, not where it was pushed inside the canvas -- and runs the model on those only; the count changes from "
             "step to step. Without this option such a job skips tiles on the fixed grid, as before. Ignored (one line) without one of the two "
             "options it builds on. Region control, wrap-around canvases and a job without a mask run as with --mdtile-grid-jitter alone; Noise "
             "Inversion's own evaluations stay on the fixed grid with every tile; DemoFusion does not read it. Default: off.")
    parser.add_argument(
        "--mdtile-region-masks", type=str, default=None, metavar="DIR",
        help="Tiled Diffusion region prompt control (MultiDiffusion, Mixture of Diffusers): free-form regions. A file DIR/region<k>.png (k = the "
             "region's number in the UI, from 1; any image Pillow reads, taken as greyscale) is region k's painted mask: the region counts "
             "exactly where at least half of a latent pixel's mask is painted, its rectangle becomes the mask's bounding box (the x, y, w, h "
             "of the UI are ignored), and a foreground region feathers along the painted shape. API callers set p.mdtile_region_masks = {k: PIL "
             "image or path}, which wins over DIR. Regions without a file stay rectangles. Refused by name: wrap-around canvases "
             "(--mdtile-wrap-x / --mdtile-wrap-y, with or without --mdtile-wrap-regions), Noise Inversion, a mask smaller than the latent canvas on "
             "either axis, and ShardedBlend (the multi-GPU blend). With --mdtile-grid-jitter and --mdtile-jitter-regions the fixed grid runs "
             "(one line); --mdtile-inpaint-skip stands down as with every region job. Default: not set, every region is a rectangle.")
