"""Alternate encoder (SAM2.1 Hiera image encoder + FPN neck, BASELINE configs[4]) on the GPU against the CPU oracle
``oracle/sam2_hiera.py`` (restatement of the sam2 package's ImageEncoder, cross-checked against the HF port in
``tests/test_cpu_oracle.py``).  Kernel-level cases first, then the whole encoder on a reduced-width Hiera with the same
head dim (72) and the same structural cases as Hiera-L."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def bf(t):
    return t.to(torch.bfloat16)


def _rows_from_grid(t):  # [D,G,G,C] -> rows
    return t.reshape(-1, t.shape[-1])


@pytest.mark.parametrize("G,ws,heads,hd,pooled", [(16, 8, 2, 72, False), (16, 8, 2, 72, True), (32, 32, 1, 72, False), (8, 4, 3, 72, False),
                                                   (8, 4, 2, 72, True), (16, 16, 2, 64, False), (16, 8, 1, 96, True), (32, 16, 2, 56, False)])
@pytest.mark.parametrize("x32", [0, 1])
def test_window_attention(gpu, G, ws, heads, hd, pooled, x32):
    """softmax(q k^T / sqrt(hd)) v inside windows; pooled: queries are the 2x2 max pool of q (Hiera stage transition).
    x32 = 1: both products on v_mfma_f32_16x16x32_bf16 (round 3; parity-tested, not the default: measured 2 % slower end to end)."""
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    _lib.set_option("win_attn_x32", x32)
    try:
        _window_attention_case(gpu, ops, G, ws, heads, hd, pooled)
    finally:
        _lib.set_option("win_attn_x32", 0)


def _window_attention_case(gpu, ops, G, ws, heads, hd, pooled):

    D, C = 3, heads * hd
    g = torch.Generator().manual_seed(G * 100 + ws + hd)
    qkv = bf(torch.randn(D, G, G, 3 * C, generator=g) * 1.5)
    rows = D * G * G
    buf = torch.zeros(ops.alloc_rows(rows), 3 * C, dtype=torch.bfloat16, device=gpu)
    buf[:rows] = _rows_from_grid(qkv).to(gpu)
    Gq, wsq = (G // 2, ws // 2) if pooled else (G, ws)
    out = torch.zeros(ops.alloc_rows(D * Gq * Gq), C + 24, dtype=torch.bfloat16, device=gpu)
    if pooled:
        qp = torch.zeros(ops.alloc_rows(D * Gq * Gq), C, dtype=torch.bfloat16, device=gpu)
        ops.pool2x2(buf, qp, slices=D, grid=G, C=C)
        qref = F.max_pool2d(qkv[..., :C].float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert torch.equal(qp[: D * Gq * Gq].float().cpu(), _rows_from_grid(qref))  # max of bf16 values: exact
        ops.window_attention(qp, 0, buf, C, 2 * C, out, slices=D, heads=heads, head_dim=hd, grid=G, window=ws, q_grid=Gq, q_window=wsq)
    else:
        qref = qkv[..., :C].float()
        ops.window_attention(buf, 0, buf, C, 2 * C, out, slices=D, heads=heads, head_dim=hd, grid=G, window=ws, q_grid=G, q_window=ws)

    def windows(t, w):  # [D,g,g,c] -> [D*nw, w*w, heads, hd]
        Dn, gg, _, c = t.shape
        t = t.reshape(Dn, gg // w, w, gg // w, w, c).permute(0, 1, 3, 2, 4, 5)
        return t.reshape(-1, w * w, heads, hd)

    q = windows(qref, wsq).transpose(1, 2)
    k = windows(qkv[..., C : 2 * C].float(), ws).transpose(1, 2)
    v = windows(qkv[..., 2 * C :].float(), ws).transpose(1, 2)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(D, Gq // wsq, Gq // wsq, wsq, wsq, C)
    ref = o.permute(0, 1, 3, 2, 4, 5).reshape(D * Gq * Gq, C)
    got = out[: D * Gq * Gq, :C].float().cpu()
    err = (got - ref).abs()
    assert err.max() <= 3e-2 and err.mean() <= 3e-3, (float(err.max()), float(err.mean()))
    assert torch.all(out[:, C:] == 0) and torch.all(out[D * Gq * Gq :] == 0)  # nothing outside the valid block is written


@pytest.mark.parametrize("G,ws,heads,hd,pooled", [(8, 4, 3, 72, False), (16, 8, 2, 72, True), (32, 16, 2, 56, False), (16, 8, 1, 96, True)])
@pytest.mark.parametrize("x32", [0, 1])
def test_window_attention_error_budget(gpu, G, ws, heads, hd, pooled, x32):
    """The rms error of hiera.hip's window attention against float64, in units of the error its documented roundings must produce
    (tests/error_budget.py; bounds from the CPU rule): 16 keys (a quarter tile), 64 keys with pooled queries, 256 keys (the online
    rescale over four tiles) at head dim 56 (rows merged in pairs), head dim 96.  Operands and band of test_window_attention."""
    import error_budget as eb
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    D, C = eb.WINDOW_D, heads * hd
    qkv = eb.window_operands(G, ws, heads, hd)
    rows = D * G * G
    buf = torch.zeros(ops.alloc_rows(rows), 3 * C, dtype=torch.bfloat16, device=gpu)
    buf[:rows] = _rows_from_grid(qkv).to(gpu)
    Gq, wsq = (G // 2, ws // 2) if pooled else (G, ws)
    out = torch.zeros(ops.alloc_rows(D * Gq * Gq), C + 24, dtype=torch.bfloat16, device=gpu)
    _lib.set_option("win_attn_x32", x32)
    try:
        if pooled:
            qp = torch.zeros(ops.alloc_rows(D * Gq * Gq), C, dtype=torch.bfloat16, device=gpu)
            ops.pool2x2(buf, qp, slices=D, grid=G, C=C)
            ops.window_attention(qp, 0, buf, C, 2 * C, out, slices=D, heads=heads, head_dim=hd, grid=G, window=ws, q_grid=Gq, q_window=wsq)
        else:
            ops.window_attention(buf, 0, buf, C, 2 * C, out, slices=D, heads=heads, head_dim=hd, grid=G, window=ws, q_grid=G, q_window=ws)
    finally:
        _lib.set_option("win_attn_x32", 0)
    fam = eb.window_case(G, ws, heads, hd, pooled, full=False)
    got = eb.window_rows(out[: D * Gq * Gq, :C].float().cpu(), Gq, wsq, heads, hd)
    err = (got - fam.ref).abs()
    assert err.max() <= 3e-2 and err.mean() <= 3e-3, (float(err.max()), float(err.mean()))
    assert torch.all(out[:, C:] == 0) and torch.all(out[D * Gq * Gq :] == 0)  # nothing outside the valid block is written
    eb.check("window_attention", f"G={G} ws={ws} heads={heads} hd={hd} pooled={pooled} x32={x32}", got, fam.ref, fam.emu)


def test_pool_cast_fpn(gpu):
    from cryovit_amd.engine import ops

    D, G, C = 2, 12, 40
    g = torch.Generator().manual_seed(1)
    x = torch.randn(D, G, G, C, generator=g)
    xin = torch.zeros(ops.alloc_rows(D * G * G), C + 8, device=gpu)
    xin[: D * G * G, :C] = _rows_from_grid(x).to(gpu)
    out = torch.zeros(ops.alloc_rows(D * 36), C, device=gpu)
    ops.pool2x2(xin, out, slices=D, grid=G, C=C)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
    assert torch.equal(out[: D * 36].cpu(), _rows_from_grid(ref))
    cb = torch.zeros(ops.alloc_rows(D * G * G), 64, dtype=torch.bfloat16, device=gpu)
    ops.cast_bf16(xin, cb, rows=D * G * G, C=C)
    assert torch.equal(cb[: D * G * G, :C].cpu(), bf(_rows_from_grid(x))) and torch.all(cb[:, C:] == 0)
    # FPN level: lateral + nearest-upsampled coarser level -> float16 [D,C,g,g]
    Cf = 72
    lat = torch.randn(D * G * G, Cf, generator=g)
    coarse = torch.randn(D * 36, Cf, generator=g)
    o16 = torch.zeros(D, Cf, G, G, dtype=torch.float16, device=gpu)
    ops.fpn_level_out(lat.to(gpu), coarse.to(gpu), o16, slices=D, C=Cf, grid=G)
    lat_i = lat.reshape(D, G, G, Cf).permute(0, 3, 1, 2)
    co_i = coarse.reshape(D, 6, 6, Cf).permute(0, 3, 1, 2)
    want = (lat_i + F.interpolate(co_i, scale_factor=2.0, mode="nearest")).half()
    assert torch.equal(o16.cpu(), want)
    ops.fpn_level_out(lat.to(gpu), None, o16, slices=D, C=Cf, grid=G)
    assert torch.equal(o16.cpu(), lat_i.half())


@pytest.mark.parametrize("H,W,dtype", [(64, 64, "u8"), (40, 56, "f32"), (100, 72, "u8"), (64, 64, "rgb")])
def test_sam_patches(gpu, H, W, dtype):
    """resize (sam2.py:196-203) + 7x7/4/3 patch gather == unfold of the oracle's resized image, to bf16 rounding."""
    from cryovit_amd.engine import ops
    from oracle import sam2_hiera as oh

    S, D = 64, 3
    rng = np.random.default_rng(H + W)
    if dtype == "u8":
        vol = torch.from_numpy(rng.integers(0, 256, (D, H, W), dtype=np.uint8))
        data = (vol.float() / 255.0)[None, :, None].repeat(1, 1, 3, 1, 1)
    elif dtype == "f32":
        vol = torch.from_numpy(rng.random((D, H, W), dtype=np.float32))
        data = vol[None, :, None].repeat(1, 1, 3, 1, 1)
    else:
        vol = torch.from_numpy(rng.random((D, 3, H, W), dtype=np.float32))
        data = vol[None]
    img = oh.resize_input(data, S)  # [D,3,S,S]
    ref = F.unfold(img, kernel_size=7, stride=4, padding=3).transpose(1, 2).reshape(D * 16 * 16, 147)
    out = torch.zeros(ops.alloc_rows(D * 256), 192, dtype=torch.bfloat16, device=gpu)
    ops.sam_patches(vol.to(gpu), out, S=S)
    got = out[: D * 256, :147].float().cpu()
    assert (got - ref).abs().max() <= 4e-3 + 1e-6  # bf16 rounding of values in [0,1]
    assert torch.all(out[:, 147:] == 0)
    if H == S and W == S:
        assert torch.equal(out[: D * 256, :147].cpu(), bf(ref))  # no resize: bit-exact


def _encoder_case(gpu, vol, cfg_name="test", fold_ln=True):
    from cryovit_amd.engine.hiera import HieraConfig, HieraEngine
    from oracle import sam2_hiera as oh

    ocfg = oh.HIERA_TEST
    cfg = HieraConfig(ocfg.embed_dim, ocfg.num_heads, ocfg.stages, ocfg.global_att_blocks, ocfg.window_spec,
                      image_size=ocfg.image_size)
    assert cfg.block_plan() == ocfg.block_plan()
    sd = oh.init_state_dict(ocfg, seed=3)
    eng = HieraEngine(cfg, {"image_encoder." + k: v for k, v in sd.items()}, gpu, fold_ln=fold_ln)  # checkpoint-style prefix
    D = vol.shape[0]
    outs = [torch.zeros(D, cfg.d_model, g, g, dtype=torch.float16, device=gpu) for g in eng.grids[: eng.n_levels()]]
    for d0 in range(0, D, 3):  # slice batches must not change the result
        eng.encode(vol[d0 : d0 + 3].to(gpu), outs, d0)
    data = (vol.float() / 255.0 if vol.dtype == torch.uint8 else vol.float())[None, :, None].repeat(1, 1, 3, 1, 1)
    ref = oh.sam_features(ocfg, sd, data)
    emu = oh.forward_features_folded_storage if fold_ln else oh.forward_features_bf16_storage  # the engine's storage plan, exact arithmetic
    ref["emu_fpn"] = [t.numpy() for t in emu(ocfg, sd, data)["backbone_fpn"]]
    return eng, outs, ref


def _check_level(lvl, got, ref, emu):
    """The ViT path's bounds (max 1e-1 / mean 1e-2 on unit-scale LayerNorm outputs) scaled to the level's mean magnitude, against the
    fp32 oracle; and against the exact-arithmetic bf16-STORAGE emulation of the same encoder the bar of the ViT headline test: the
    kernels sit no further from the emulation than the emulation sits from fp32 (two implementations of one storage plan)."""
    scale = max(1.0, float(np.abs(ref).mean()))
    e_f32, e_emu, e_store = np.abs(got - ref), np.abs(got - emu), np.abs(emu - ref)
    stats = (lvl, scale, float(e_f32.max()), float(e_f32.mean()), float(e_emu.max()), float(e_emu.mean()), float(e_store.max()), float(e_store.mean()))
    print("hiera level %d (scale %.2f): vs fp32 max %.3e mean %.3e; vs bf16-storage emulation max %.3e mean %.3e; emulation vs fp32 max %.3e mean %.3e" % stats)
    assert e_f32.max() <= 0.1 * scale and e_f32.mean() <= 0.01 * scale, stats
    assert e_emu.mean() <= e_store.mean() + 1e-4 and e_emu.max() <= 1.25 * e_store.max() + 1e-2 * scale, stats


@pytest.mark.parametrize("fold_ln", [True, False])
@pytest.mark.parametrize("H", [128, 96])
def test_hiera_encoder_vs_oracle(gpu, H, fold_ln):
    """Whole image encoder (patch embed, 8 blocks incl. three q-pooled transitions and global blocks, 4-level neck with the
    top-down path, scalp) vs the fp32 oracle; H = 96 exercises the bilinear resize to the encoder's 128x128."""
    rng = np.random.default_rng(H)
    vol = torch.from_numpy(rng.integers(0, 256, (4, H, H), dtype=np.uint8))
    eng, outs, ref = _encoder_case(gpu, vol, fold_ln=fold_ln)
    assert [tuple(o.shape) for o in outs] == [(4, 256, 32, 32), (4, 256, 16, 16), (4, 256, 8, 8)]
    for lvl, (o, r) in enumerate(zip(outs, ref["backbone_fpn"])):
        # bf16 GEMM operands / fp32 accumulation and residual stream: the ViT path's tolerance (round 3: was 1.5x / 2x of it)
        _check_level(lvl, o.float().cpu().numpy(), r.astype(np.float32), ref["emu_fpn"][lvl])
    for lvl, r in enumerate(ref["vision_pos_enc"]):
        assert torch.equal(eng.pos_enc(lvl), torch.from_numpy(r[0]))  # input independent: bit-exact fp16


def test_sam_features_entry_point_hiera_l(gpu, tmp_path):
    """BASELINE configs[4] plumbing: ``python -m ...training.sam_features`` on a synthetic data directory with the full
    Hiera-L encoder (seeded random weights), output layout of ``_save_data`` (run/dino_features.py:133-146) and values
    against the CPU oracle on two slices.  The 256x256 tomogram is resized to the encoder's 512x512 on the GPU."""
    from cryovit_amd import io
    from cryovit_amd.engine.hiera import HIERA_CONFIGS, random_state_dict
    from cryovit_amd.training import sam_features
    from oracle import sam2_hiera as oh

    rng = np.random.default_rng(4)
    vol = rng.integers(0, 256, size=(5, 256, 256), dtype=np.uint8)
    lab = rng.integers(-1, 2, size=vol.shape).astype(np.int8)
    old = rng.standard_normal((8, 5, 2, 2)).astype(np.float16)
    src = tmp_path / "processed" / "Q109"
    src.mkdir(parents=True)
    with io.FileWriter(src / "tomo_a.hdf") as f:
        f.create_dataset("data", vol, compression="gzip")
        f.create_dataset("labels/mito", lab, compression="gzip")
        f.create_dataset("dino_features", old)
    sam_features.main([f"paths.model_dir={tmp_path}", f"paths.data_dir={tmp_path}", f"paths.exp_dir={tmp_path / 'exp'}",
                       "paths.feature_name=processed", "sample=Q109", "batch_size=4", "encoder.synthetic_seed=7"])
    out = tmp_path / "tomograms" / "Q109" / "tomo_a.hdf"
    assert out.exists(), "entry point did not produce the output tomogram (see logged traceback)"
    assert sorted(io.list_keys(out)) == ["data", "dino_features", "labels", "sam_features"]
    assert sorted(io.list_keys(out, "sam_features")) == ["backbone_fpn", "vision_pos_enc"]
    assert np.array_equal(io.read_dataset(out, "data"), vol) and np.array_equal(io.read_dataset(out, "labels/mito"), lab)
    assert np.array_equal(io.read_dataset(out, "dino_features"), old)  # the source's DINO features are kept (l.136-138)
    cfg = HIERA_CONFIGS["sam2.1_hiera_l"]
    sd = {k: v.cpu() for k, v in random_state_dict(cfg, 7, device=gpu).items()}
    assert oh.HIERA_L.block_plan() == cfg.block_plan()
    pick = [0, 4]  # both sides of the slice batch of 4
    data = torch.from_numpy(vol[pick].astype(np.float32) / 255.0)[None, :, None].repeat(1, 1, 3, 1, 1)
    ref = oh.sam_features(oh.HIERA_L, sd, data)
    emu = [t.numpy() for t in oh.forward_features_folded_storage(oh.HIERA_L, sd, data)["backbone_fpn"]]  # the shipped storage plan
    for lvl, g in enumerate((128, 64, 32)):
        got = io.read_dataset(out, f"sam_features/backbone_fpn/{lvl}")
        assert got.dtype == np.float16 and got.shape == (5, 256, g, g)
        _check_level(lvl, got[pick].astype(np.float32), ref["backbone_fpn"][lvl].astype(np.float32), emu[lvl])
        pos = io.read_dataset(out, f"sam_features/vision_pos_enc/{lvl}")
        assert pos.dtype == np.float16 and pos.shape == (5, 256, g, g) and np.array_equal(pos[pick], ref["vision_pos_enc"][lvl])


def test_sam_protocol_forward_features(gpu):
    """``model.forward_features(data [1,D,3,H,W])`` (the reference's call, run/dino_features.py:91) == the fused raw path."""
    from cryovit_amd.models import load_sam_encoder
    from cryovit_amd.run.dino_features import _sam_features

    enc = load_sam_encoder("SAM2", synthetic_seed=5, device=gpu, slice_batch=2)
    rng = np.random.default_rng(8)
    vol = torch.from_numpy(rng.random((3, 512, 512), dtype=np.float32))
    fused = _sam_features(vol, enc, 128)
    proto = _sam_features(vol[None, :, None].repeat(1, 1, 3, 1, 1), enc, 128)
    assert list(fused) == list(proto) == ["vision_pos_enc", "backbone_fpn"]
    for key in fused:
        for a, b in zip(fused[key], proto[key]):
            assert a.dtype == b.dtype == np.float16 and a.shape == b.shape and np.array_equal(a, b)
