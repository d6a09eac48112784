"""Tiled VAE on several device slots of one process (VAEHook.devices, --mdtile-devices): every mode bit-identical to one device, the tile
assembly kernel (mdtile_vae_assemble) against one crop_store per tile, the host's error paths, the plugin switch and the weight cache.
On one GPU the slots are cuda:0 listed several times; [0, 1] runs where two GPUs are visible."""
import pytest
import torch

from hostsim import ldm_decoder as ld

pytestmark = pytest.mark.gpu

SLOTS = [[0, 0], [0, 0, 0],
         pytest.param([0, 1], marks=pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two visible GPUs"))]


def _enc_size(n: int) -> int:
    for _ in range(3):                  # the encoder's three ldm Downsample convs (pad right / bottom by 1, 3x3 stride 2)
        n = (n - 2) // 2 + 1
    return n


def _tiles(E, h, w, ts, is_decoder, N, C, narrow=False, seed=0):
    ins, outs = E.vae_split_tiles(h, w, ts, is_decoder)
    g = torch.Generator(device="cpu").manual_seed(seed)
    tiles = []
    for ib, ob in zip(ins, outs):
        if narrow:                      # a live-window input bbox: the tile shrunk to its valid rectangle grown by 1 latent px
            x1, x2, y1, y2 = ib
            ib = [max(x1, ob[0] // 8 - 1), min(x2, ob[1] // 8 + 1), max(y1, ob[2] // 8 - 1), min(y2, ob[3] // 8 + 1)]
        th, tw = ((ib[3] - ib[2]) * 8, (ib[1] - ib[0]) * 8) if is_decoder else (_enc_size(ib[3] - ib[2]), _enc_size(ib[1] - ib[0]))
        tiles.append((torch.randn(N, C, th, tw, generator=g).cuda(), ib, ob))
    shape = (N, C, h * 8, w * 8) if is_decoder else (N, C, h // 8, w // 8)
    return tiles, shape


@pytest.mark.parametrize("h,w,ts,is_decoder,N,C,narrow", [
    (64, 64, 16, True, 1, 3, False),           # decoder geometry: windows at multiples of 8 px
    (64, 64, 16, True, 2, 3, True),            # batch 2, narrowed live-window input bboxes
    (136, 120, 16, True, 1, 3, False),         # 56 tiles: more than one chunk of the kernel-argument table
    (200, 264, 64, False, 1, 8, False),        # encoder geometry: margins from a division by 8 (unaligned rows)
    (256, 328, 64, False, 2, 8, False),
], ids=["decoder", "decoder_b2_live", "decoder_two_chunks", "encoder", "encoder_b2"])
def test_vae_assemble_matches_crop_store(plugin, cuda, h, w, ts, is_decoder, N, C, narrow):
    E = plugin.engine
    tiles, shape = _tiles(E, h, w, ts, is_decoder, N, C, narrow)
    if h == 136:
        assert len(tiles) > E.VAE_ASSEMBLE_CHUNK
    want = torch.full(shape, -7.0, device=cuda)
    for t, ib, ob in tiles:
        E.crop_store(t, ib, ob, want, is_decoder)
    got = torch.full(shape, -7.0, device=cuda)
    E.vae_assemble(tiles, got, is_decoder)
    assert torch.equal(got, want)


def test_vae_assemble_rejects_bad_bboxes(plugin, cuda):
    E = plugin.engine
    tiles, shape = _tiles(E, 64, 64, 16, True, 1, 3)
    out = torch.zeros(shape, device=cuda)
    t, ib, ob = tiles[1]
    with pytest.raises(E.MdtileError, match="inconsistent bboxes"):
        E.vae_assemble(tiles[:1] + [(t, ib, [ob[0] - 200, ob[1], ob[2], ob[3]])], out, True)
    with pytest.raises(E.MdtileError, match="outside the result"):
        E.vae_assemble([(t, ib, ob)], torch.zeros(1, 3, 64, 64, device=cuda), True)
    assert not out.any()                       # an error return launches nothing


def _decoder(seed=4, small=False):
    dec = ld.make_decoder(seed, small=small).cuda()
    dec.original_forward = dec.forward
    return dec


def _both(hook, x, slots):
    hook.devices = None
    one = hook(x).clone()
    hook.devices = list(slots)
    many = hook(x)
    return one, many


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("fast", [True, False], ids=["fast", "slow"])
def test_decode_on_slots_is_bit_identical(plugin, cuda, slots, fast):
    dec = _decoder()
    torch.manual_seed(13)
    z = torch.randn(1, 4, 64, 64, device=cuda)              # 9 tiles at tile 16
    hook = plugin.tilevae.VAEHook(dec, 16, is_decoder=True, fast_decoder=fast, fast_encoder=False, color_fix=False)
    one, many = _both(hook, z, slots)
    assert many.device == one.device and many.dtype == one.dtype and torch.equal(many, one)
    assert len(hook.last_tile_slots) == 9 and set(hook.last_tile_slots) == set(range(len(slots)))


@pytest.mark.parametrize("slots", SLOTS)
@pytest.mark.parametrize("fast,color_fix", [(True, False), (False, False), (True, True)], ids=["fast", "slow", "color_fix"])
def test_encode_on_slots_is_bit_identical(plugin, cuda, slots, fast, color_fix):
    enc = ld.make_encoder(2, small=True).cuda()
    enc.original_forward = enc.forward
    torch.manual_seed(6)
    x = torch.randn(1, 3, 200, 264, device=cuda)            # 12 tiles at tile 64
    hook = plugin.tilevae.VAEHook(enc, 64, is_decoder=False, fast_decoder=False, fast_encoder=fast, color_fix=color_fix)
    one, many = _both(hook, x, slots)
    assert torch.equal(many, one)
    assert len(hook.last_tile_slots) == 12 and set(hook.last_tile_slots) == set(range(len(slots)))


def test_half_precision_vae_and_bf16_mode_on_slots(plugin, cuda):
    E = plugin.engine
    dec = ld.make_decoder(6, small=True).half().cuda()
    dec.original_forward = dec.forward
    torch.manual_seed(9)
    z = torch.randn(1, 4, 64, 64, device=cuda).half()
    hook = plugin.tilevae.VAEHook(dec, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    one, many = _both(hook, z, [0, 0])
    assert many.dtype == torch.float16 and torch.equal(many, one)
    dec32 = _decoder(6, small=True)
    hook = plugin.tilevae.VAEHook(dec32, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    with E.precision(E.PRECISION_BF16):
        one, many = _both(hook, z.float(), [0, 0, 0])
    assert torch.equal(many, one)


def test_nan_raises_the_hosts_exception_on_slots(plugin, cuda):
    import modules.devices as host_devices
    dec = _decoder(4, small=True)
    z = torch.randn(1, 4, 64, 64, device=cuda)
    z[0, 1, 20, 30] = float("nan")
    hook = plugin.tilevae.VAEHook(dec, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    with pytest.raises(host_devices.NansException):
        hook(z)
    hook.devices = [0, 0]
    with pytest.raises(host_devices.NansException):
        hook(z)


@pytest.mark.parametrize("is_decoder", [True, False], ids=["decoder", "encoder"])
def test_interrupt_before_the_call_matches_one_device(plugin, cuda, is_decoder):
    import modules.shared as shared
    net = (ld.make_decoder(4, small=True) if is_decoder else ld.make_encoder(2, small=True)).cuda()
    net.original_forward = net.forward
    x = torch.randn(1, 4, 64, 64, device=cuda) if is_decoder else torch.randn(1, 3, 200, 264, device=cuda)
    hook = plugin.tilevae.VAEHook(net, 16 if is_decoder else 64, is_decoder=is_decoder, fast_decoder=True, fast_encoder=True, color_fix=False)
    shared.state.interrupted = True
    try:
        if is_decoder:
            one, many = _both(hook, x, [0, 0])
            assert torch.equal(many, one)
        else:
            with pytest.raises(RuntimeError, match="interrupted"):
                hook(x)
            hook.devices = [0, 0]
            with pytest.raises(RuntimeError, match="interrupted"):
                hook(x)
    finally:
        shared.state.interrupted = False


def test_slots_and_a_process_shard_do_not_mix(plugin, cuda):
    hook = plugin.tilevae.VAEHook(_decoder(4, small=True), 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
    hook.devices, hook.shard = [0, 0], (0, 2)
    with pytest.raises(RuntimeError, match="cannot be combined"):
        hook(torch.randn(1, 4, 64, 64, device=cuda))


def test_plugin_switch_arms_both_hooks(plugin, cuda, monkeypatch):
    from types import SimpleNamespace
    import modules.shared as shared
    tv = plugin.tilevae
    dec = _decoder(4, small=True)
    enc = ld.make_encoder(2, small=True).cuda()
    p = SimpleNamespace(sd_model=SimpleNamespace(first_stage_model=SimpleNamespace(encoder=enc, decoder=dec)))
    monkeypatch.setattr(shared.cmd_opts, "mdtile_devices", "0,0", raising=False)
    s = tv.Script()
    try:
        s.process(p, True, 64, 16, False, True, True, False)
        assert dec.forward.devices == [0, 0] and enc.forward.devices == [0, 0]
        torch.manual_seed(3)
        z = torch.randn(1, 4, 64, 64, device=cuda)
        many = dec.forward(z).clone()
        assert set(dec.forward.last_tile_slots) == {0, 1}
        dec.forward.devices = None
        assert torch.equal(dec.forward(z), many)
        monkeypatch.setattr(shared.cmd_opts, "mdtile_devices", None)
        s.process(p, True, 64, 16, False, True, True, False)
        assert dec.forward.devices is None and enc.forward.devices is None
    finally:
        s.postprocess(p, None, True)


def test_slot_programs_are_cached_per_set_of_weights(plugin, cuda, monkeypatch):
    tv = plugin.tilevae
    builds = []
    real = tv.build_task_queue

    def counting(net, *a, **k):
        builds.append(net)
        return real(net, *a, **k)

    monkeypatch.setattr(tv, "build_task_queue", counting)
    dec = _decoder(4, small=True)
    torch.manual_seed(5)
    z = torch.randn(1, 4, 64, 64, device=cuda)

    def hook():
        h = tv.VAEHook(dec, 16, is_decoder=True, fast_decoder=True, fast_encoder=False, color_fix=False)
        h.devices = [0, 0]
        return h

    first = hook()(z).clone()
    assert len(builds) == 2                    # the hook's own program + the program of slot 1
    again = hook()(z)
    assert len(builds) == 3                    # a second hook (the next generation) builds only its own program
    assert torch.equal(again, first)
    dec.load_state_dict(ld.make_decoder(8, small=True).state_dict())       # an in-place VAE swap
    h = hook()
    many = h(z).clone()
    assert len(builds) == 5                    # own program + slot 1 rebuilt for the new weights
    h.devices = None
    one = h(z)
    assert torch.equal(many, one) and not torch.equal(many, first)
