"""Alternate encoder (SAM2.1 Hiera image encoder + FPN neck, BASELINE configs[4]) on the GPU against the CPU oracle
``oracle/sam2_hiera.py`` (restatement of the sam2 package's ImageEncoder, cross-checked against the HF port in
``tests/test_cpu_oracle.py``).  Kernel-level cases first, then the whole encoder on a reduced-width Hiera with the same
head dim (72) and the same structural cases as Hiera-L."""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import error_budget as eb

pytestmark = pytest.mark.gpu


def bf(t):
    return t.to(torch.bfloat16)


def _rows_from_grid(t):  # [D,G,G,C] -> rows
    return t.reshape(-1, t.shape[-1])


SENTINEL = 0.3331  # fills every output buffer and pad column (tests/test_gpu_unet_backward.py): a kernel must leave it alone


def _sentinel(shape, dtype, gpu):
    return torch.full(shape, SENTINEL, dtype=dtype, device=gpu)


def _untouched(t):
    return bool((t == torch.tensor(SENTINEL, dtype=t.dtype)).all())


def _nan_rows(data, alloc, width, gpu):
    """`data` [rows, c] in the leading corner of a NaN buffer [alloc, width]: a read of a slack row or a pad column shows in the output."""
    buf = torch.full((alloc, width), float("nan"), dtype=data.dtype)
    buf[: data.shape[0], : data.shape[1]] = data
    return buf.to(gpu)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32}[t.element_size()])


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


def _run_window(gpu, qkv, G, ws, heads, hd, pooled):
    """qkv bf16 [D, G, G, 3 C] -> the kernel's output rows [D Gq Gq, C] (bf16, CPU).  k and v at columns C and 2 C of the row buffer, q
    at column 0 of it or, pooled, of cvx_pool2x2's output.  Input slack rows hold NaN, the output's slack rows and pad columns the
    sentinel, which must survive."""
    from cryovit_amd.engine import ops

    D, C = qkv.shape[0], heads * hd
    rows = D * G * G
    buf = _nan_rows(_rows_from_grid(qkv), ops.alloc_rows(rows), 3 * C, gpu)
    Gq, wsq = (G // 2, ws // 2) if pooled else (G, ws)
    nrow = D * Gq * Gq
    out = _sentinel((ops.alloc_rows(nrow), C + 24), torch.bfloat16, gpu)
    if pooled:
        qp = torch.full((ops.alloc_rows(nrow), C), float("nan"), dtype=torch.bfloat16, device=gpu)
        ops.pool2x2(buf, qp, slices=D, grid=G, C=C)
        qref = F.max_pool2d(qkv[..., :C].float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert torch.equal(qp[:nrow].float().cpu(), _rows_from_grid(qref))  # max of bf16 values: exact
        ops.window_attention(qp, 0, buf, C, 2 * C, out, slices=D, heads=heads, head_dim=hd, grid=G, window=ws, q_grid=Gq, q_window=wsq)
    else:
        ops.window_attention(buf, 0, buf, C, 2 * C, out, slices=D, heads=heads, head_dim=hd, grid=G, window=ws, q_grid=G, q_window=ws)
    assert _untouched(out[:, C:]) and _untouched(out[nrow:])  # nothing outside the valid block is written
    return out[:nrow, :C].cpu()


def _window_attention_case(gpu, ops, G, ws, heads, hd, pooled):
    D, C = 3, heads * hd
    g = torch.Generator().manual_seed(G * 100 + ws + hd)
    qkv = bf(torch.randn(D, G, G, 3 * C, generator=g) * 1.5)
    Gq, wsq = (G // 2, ws // 2) if pooled else (G, ws)
    got = _run_window(gpu, qkv, G, ws, heads, hd, pooled).float()
    qref = F.max_pool2d(qkv[..., :C].float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1) if pooled else qkv[..., :C].float()

    def windows(t, w):  # [D,g,g,c] -> [D*nw, w*w, heads, hd]
        Dn, gg, _, c = t.shape
        t = t.reshape(Dn, gg // w, w, gg // w, w, c).permute(0, 1, 3, 2, 4, 5)
        return t.reshape(-1, w * w, heads, hd)

    q = windows(qref, wsq).transpose(1, 2)
    k = windows(qkv[..., C : 2 * C].float(), ws).transpose(1, 2)
    v = windows(qkv[..., 2 * C :].float(), ws).transpose(1, 2)
    o = F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(D, Gq // wsq, Gq // wsq, wsq, wsq, C)
    ref = o.permute(0, 1, 3, 2, 4, 5).reshape(D * Gq * Gq, C)
    err = (got - ref).abs()
    assert err.max() <= 3e-2 and err.mean() <= 3e-3, (float(err.max()), float(err.mean()))


def _check_window(label, got_rows, fam, Gq, wsq, heads, hd):
    """The elementwise band of test_window_attention and the window bounds of tests/error_budget.py on one result."""
    got = eb.window_rows(got_rows.float(), Gq, wsq, heads, hd)
    err = (got - fam.ref).abs()
    assert err.max() <= 3e-2 and err.mean() <= 3e-3, (float(err.max()), float(err.mean()))
    return eb.check("window_attention", label, got, fam.ref, fam.emu)


@pytest.mark.parametrize("G,ws,heads,hd,pooled", [(8, 4, 3, 72, False), (16, 8, 2, 72, True), (32, 16, 2, 56, False), (16, 8, 1, 96, True)])
@pytest.mark.parametrize("x32", [0, 1])
def test_window_attention_error_budget(gpu, G, ws, heads, hd, pooled, x32):
    """The rms error of hiera.hip's window attention against float64, in units of the error its documented roundings must produce
    (tests/error_budget.py; bounds from the CPU rule): 16 keys (a quarter tile), 64 keys with pooled queries, 256 keys (the online
    rescale over four tiles) at head dim 56 (rows merged in pairs), head dim 96.  Operands and band of test_window_attention."""
    from cryovit_amd import _lib

    Gq, wsq = (G // 2, ws // 2) if pooled else (G, ws)
    _lib.set_option("win_attn_x32", x32)
    try:
        got = _run_window(gpu, eb.window_operands(G, ws, heads, hd), G, ws, heads, hd, pooled)
    finally:
        _lib.set_option("win_attn_x32", 0)
    fam = eb.window_case(G, ws, heads, hd, pooled, full=False)
    _check_window(f"G={G} ws={ws} heads={heads} hd={hd} pooled={pooled} x32={x32}", got, fam, Gq, wsq, heads, hd)


@pytest.fixture
def win_options():
    """set(prefetch, x32) for the window kernel's two options; the defaults (1, 0) are put back whatever happens."""
    from cryovit_amd import _lib

    def set_(prefetch, x32):
        _lib.set_option("win_attn_prefetch", prefetch)
        _lib.set_option("win_attn_x32", x32)

    try:
        yield set_
    finally:
        _lib.set_option("win_attn_prefetch", 1)
        _lib.set_option("win_attn_x32", 0)


@pytest.mark.parametrize("G,ws,heads,hd,pooled", [pytest.param(*c, id="-".join(str(v) for v in c)) for c in eb.WINDOW_DISPATCH_CASES + eb.WINDOW_CASES])
@pytest.mark.parametrize("x32", [0, 1])
@pytest.mark.parametrize("prefetch", [0, 1, 2])
def test_window_attention_dispatch(gpu, win_options, G, ws, heads, hd, pooled, prefetch, x32):
    """cvx_window_attention_bf16 on every template form it can launch: plain, PF, PF2, X32, X32+PF, each at DSTEPS 4, 5 and 6
    (error_budget.window_form names the form a (case, options) pair takes; tests/test_cpu_error_budget.py asserts that the cases cover
    all fifteen and both branches of the block renumbering).  The dispatch cases add the windows that are no power of two (kl / ws,
    kl % ws addressing; a ragged last query block; waves without a valid query), the head dims with hd % 8 != 0 at full blocks, the
    smallest head dim, and 1024 keys.  Key tiles of 32 and 48 keys (nsub 2 and 3) cannot occur: nk = ws^2 is a multiple of 16, and
    ws^2 mod 64 is 0, 16 or (ws odd: refused) -- never 32 or 48.  Checks: the elementwise band, the window bounds against the float64
    family, sentinel slack, NaN input slack."""
    form, ds, _ = eb.window_form(G, ws, heads, hd, pooled, prefetch, x32)
    Gq, wsq = (G // 2, ws // 2) if pooled else (G, ws)
    win_options(prefetch, x32)
    got = _run_window(gpu, eb.window_operands(G, ws, heads, hd), G, ws, heads, hd, pooled)
    fam = eb.window_case(G, ws, heads, hd, pooled, full=False)
    _check_window(f"G={G} ws={ws} heads={heads} hd={hd} pooled={pooled} prefetch={prefetch} x32={x32} {form}/{ds}", got, fam, Gq, wsq, heads, hd)


@pytest.mark.parametrize("G,ws,heads,hd,pooled,x32", [(32, 16, 1, 80, False, 0), (32, 32, 1, 88, False, 0), (16, 16, 2, 64, True, 1)])
def test_window_attention_prefetch_changes_staging_only(gpu, win_options, G, ws, heads, hd, pooled, x32):
    """plain, PF and PF2 (x32 = 1: X32, X32+PF) stage the same K / V tiles in different ways and run the same MFMAs in the same
    order: bit-identical outputs."""
    forms, outs = [], []
    for prefetch in eb.WINDOW_PREFETCH:
        win_options(prefetch, x32)
        forms.append(eb.window_form(G, ws, heads, hd, pooled, prefetch, x32)[0])
        outs.append(_run_window(gpu, eb.window_operands(G, ws, heads, hd), G, ws, heads, hd, pooled))
    assert forms == (["X32", "X32+PF", "X32+PF"] if x32 else ["plain", "PF", "PF2"])
    assert torch.equal(_bits(outs[0]), _bits(outs[1])) and torch.equal(_bits(outs[0]), _bits(outs[2]))


@pytest.mark.parametrize("spike", [0.25, 9.0])
@pytest.mark.parametrize("prefetch", [0, 1, 2])
def test_window_attention_forced_rescale(gpu, win_options, prefetch, spike):
    """In every window key 150 = spike * query 7: the running maximum of about half the rows jumps in the third of four key tiles, so
    the accumulated output must be rescaled there (hiera.hip:253-254, :294).  Band and window bounds against the "running" family;
    on the CPU the honest R_row is at most 1.717 and an output that is not rescaled has R_all above 400."""
    G, ws, heads, hd, pooled = eb.WINDOW_RESCALE_CASE
    win_options(prefetch, 0)
    got = _run_window(gpu, eb.window_rescale_operands(spike), G, ws, heads, hd, pooled)
    _check_window(f"forced rescale spike={spike} prefetch={prefetch}", got, eb.window_rescale_case(spike, full=False), G, ws, heads, hd)


def test_window_attention_refusals(gpu):
    """Every argument the entry has no kernel for returns the argument error, names window_attention in cvx_last_error and leaves the
    output as it was; slices = 0 is a no-op that returns 0."""
    from cryovit_amd import _lib

    lib = _lib.load()
    G, ws, heads, hd = 16, 8, 2, 8
    C = heads * hd
    buf = _nan_rows(bf(torch.randn(G * G, 3 * C, generator=torch.Generator().manual_seed(5))), 1024, 3 * C, gpu)
    out = _sentinel((1024, C + 24), torch.bfloat16, gpu)
    ok = dict(ldq=3 * C, ldkv=3 * C, ldo=C + 24, slices=1, heads=heads, hd=hd, grid=G, window=ws, q_grid=G, q_window=ws)

    def run(**kw):
        a = dict(ok, **kw)
        with torch.cuda.device(out.device):
            rc = lib.cvx_window_attention_bf16(buf.data_ptr(), a["ldq"], buf.data_ptr() + 2 * C, buf.data_ptr() + 4 * C, a["ldkv"], out.data_ptr(),
                                               a["ldo"], a["slices"], a["heads"], a["hd"], a["grid"], a["window"], a["q_grid"], a["q_window"],
                                               torch.cuda.current_stream(out.device).cuda_stream)
        torch.cuda.synchronize()
        return rc

    refused = {"window 6: 36 keys, no multiple of 16": dict(grid=12, window=6, q_grid=12, q_window=6),
               "hd 6": dict(hd=6), "hd 100": dict(hd=100), "hd 70": dict(hd=70),
               "ldq % 4": dict(ldq=3 * C + 2), "ldkv % 4": dict(ldkv=3 * C + 2), "ldo % 4": dict(ldo=C + 26),
               "grid the window does not divide": dict(grid=20), "query grid its window does not divide": dict(q_grid=12),
               "unequal window counts": dict(q_window=4),
               "nwin * heads > 65535": dict(grid=1024, window=4, q_grid=1024, q_window=4, heads=1),
               "nwin * heads > 65535, by the heads": dict(grid=512, window=4, q_grid=512, q_window=4, heads=4)}
    for name, kw in refused.items():
        rc = run(**kw)
        assert rc != 0 and b"window_attention" in lib.cvx_last_error(), (name, rc, lib.cvx_last_error())
        assert _untouched(out), f"{name}: a refused call wrote the output"
    assert run(slices=0) == 0 and _untouched(out)
    assert run() == 0 and not _untouched(out[: G * G, :C]) and _untouched(out[:, C:]) and _untouched(out[G * G :])  # (the base call is valid)


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
    out = _sentinel((ops.alloc_rows(D * 256), 192), torch.bfloat16, gpu)
    ops.sam_patches(vol.to(gpu), out, S=S)
    got = out[: D * 256, :147].float().cpu()
    assert (got - ref).abs().max() <= 4e-3 + 1e-6  # bf16 rounding of values in [0,1]
    assert _untouched(out[:, 147:]) and _untouched(out[D * 256 :])  # the kernel writes no column at or past 147
    if H == S and W == S:
        assert torch.equal(out[: D * 256, :147].cpu(), bf(ref))  # no resize: bit-exact


def _slack_volume(vol, gpu):
    """`vol` on the device with NaN (uint8: 255) behind its last element, so that a read past the volume shows."""
    fill = 255 if vol.dtype == torch.uint8 else float("nan")
    flat = torch.full((vol.numel() + 256,), fill, dtype=vol.dtype)
    flat[: vol.numel()] = vol.reshape(-1)
    return flat.to(gpu)[: vol.numel()].view(vol.shape)


@pytest.mark.parametrize("ldo", [160, 192, 256])
@pytest.mark.parametrize("D", [1, 5])
@pytest.mark.parametrize("S,H,W,mode", [pytest.param(*c, id="-".join(str(v) for v in c)) for c in eb.SAM_PATCH_CASES])
def test_sam_patches_bound(gpu, S, H, W, mode, D, ldo):
    """cvx_sam_patches against the float64 closed form of resize + gather (error_budget.sam_patches_reference, pinned against the
    oracle on the CPU), elementwise:  |got - ref64| <= half a bf16 ulp at ref64 + e32, with e32 the fp32 term derived there from the
    source coordinate and the four-tap sum (at most 1.7e-5 here; half an ulp of a value near 1 is 2e-3, so no second ulp is allowed
    anywhere).  Without a resize the output is the bf16 rounding of the source, bit for bit; taps outside the image are exactly 0;
    columns 147.. of every leading dimension and the rows behind the last patch keep their sentinel (the kernel writes neither)."""
    from cryovit_amd.engine import ops

    vol = eb.sam_volume(D, H, W, mode)
    ref, e32, inside = eb.sam_patches_reference(vol, S)
    rows = D * (S // 4) ** 2
    out = _sentinel((ops.alloc_rows(rows), ldo), torch.bfloat16, gpu)
    ops.sam_patches(_slack_volume(vol, gpu), out, S=S)
    got = out[:rows, :147].cpu()
    assert _untouched(out[:, 147:]) and _untouched(out[rows:])
    err, bound = (got.double() - ref).abs(), eb.rounded_store_bound(ref, e32)
    print(f"sam_patches S={S} {H}x{W} {mode} D={D} ldo={ldo}: e32 {e32:.2e}, max err / bound {float((err / bound).max()):.3f}")
    assert not bool(torch.isnan(got.float()).any())
    assert bool((got.float()[~inside] == 0).all())
    assert bool((err <= bound).all()), float((err / bound).max())
    if e32 == 0.0:
        assert torch.equal(_bits(got), _bits(bf(ref.float())))


def test_sam_patches_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    vol = torch.zeros(1, 16, 16, device=gpu)
    out = _sentinel((ops.alloc_rows(16), 160), torch.bfloat16, gpu)
    for S in (18, 0):
        with pytest.raises(_lib.CvxError, match="sam_patches"):
            ops.sam_patches(vol, out, S=S)
    with pytest.raises(_lib.CvxError, match="sam_patches"):
        ops.sam_patches(vol, out[:, :144].contiguous(), S=16)  # a row too narrow for 147 taps
    torch.cuda.synchronize()
    assert _untouched(out)


# ---- pool, cast, FPN level output, stream merge: bit-exact against torch ------------------------------------------------------------------


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [1, 3])
@pytest.mark.parametrize("C", [4, 12, 72])
@pytest.mark.parametrize("G", [2, 6])
def test_pool2x2_exact(gpu, G, C, D, dtype):
    """2x2 max pool over the token grid, both element types, leading dimensions wider than C on both sides: the bits of
    F.max_pool2d (operands without NaN and without zeros, so the maximum is one of the inputs whatever the comparison's order)."""
    from cryovit_amd.engine import ops

    x = (torch.randn(D, G, G, C, generator=torch.Generator().manual_seed(G * 100 + C + D)) * 2).to(dtype)
    assert not bool((x == 0).any())
    Go = G // 2
    xin = _nan_rows(_rows_from_grid(x), ops.alloc_rows(D * G * G), C + 8, gpu)
    out = _sentinel((ops.alloc_rows(D * Go * Go), C + 12), dtype, gpu)
    ops.pool2x2(xin, out, slices=D, grid=G, C=C)
    ref = F.max_pool2d(x.float().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).to(dtype)
    assert torch.equal(_bits(out[: D * Go * Go, :C].cpu()), _bits(_rows_from_grid(ref)))
    assert _untouched(out[:, C:]) and _untouched(out[D * Go * Go :])


def test_pool2x2_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    x = torch.zeros(256, 16, device=gpu)
    out = _sentinel((256, 16), torch.float32, gpu)
    for kw in (dict(grid=3, C=8), dict(grid=2, C=6)):
        with pytest.raises(_lib.CvxError, match="pool2x2"):
            ops.pool2x2(x, out, slices=1, **kw)
    with pytest.raises(_lib.CvxError, match="pool2x2"):
        ops.pool2x2(torch.zeros(256, 18, device=gpu), out, slices=1, grid=2, C=8)
    torch.cuda.synchronize()
    assert _untouched(out)


# round-to-nearest-even ties in both directions (1 + 2^-8 -> 1, 1 + 3 2^-8 -> 1 + 2^-6), either sign; signed zeros; fp32 subnormals (one
# a bf16 subnormal, one that rounds to zero); the largest finite fp32 (rounds to inf); infinities
CAST_CRAFTED = [1.0 + 2.0**-8, 1.0 + 3 * 2.0**-8, -(1.0 + 2.0**-8), -(1.0 + 3 * 2.0**-8), 0.0, -0.0, 2.0**-133, -(2.0**-130), 2.0**-149,
                3.4028234663852886e38, -3.4028234663852886e38, float("inf"), -float("inf"), 1.0 + 2.0**-8 + 2.0**-20, 1.0 + 2.0**-8 - 2.0**-20]


@pytest.mark.parametrize("C", [4, 144])
@pytest.mark.parametrize("rows", [1, 37])
def test_cast_bf16_exact(gpu, rows, C):
    """fp32 -> bf16, the bits of tensor.to(torch.bfloat16): random values, and the crafted values above at the end of the matrix
    (rows = 1, C = 4 holds the four ties)."""
    from cryovit_amd.engine import ops

    x = torch.randn(rows, C, generator=torch.Generator().manual_seed(rows + C)) * 3
    n = min(x.numel(), len(CAST_CRAFTED))
    x.view(-1)[x.numel() - n :] = torch.tensor(CAST_CRAFTED[:n])
    xin = _nan_rows(x, ops.alloc_rows(rows), C + 4, gpu)
    out = _sentinel((ops.alloc_rows(rows), C + 8), torch.bfloat16, gpu)
    ops.cast_bf16(xin, out, rows=rows, C=C)
    assert torch.equal(_bits(out[:rows, :C].cpu()), _bits(bf(x)))
    assert _untouched(out[:, C:]) and _untouched(out[rows:])


@pytest.mark.parametrize("g,C,with_coarse", [(1, 8, False), (9, 130, False), (2, 8, True), (4, 256, True), (10, 130, True)])
def test_fpn_level_out_exact(gpu, g, C, with_coarse):
    """lateral (+ the nearest-upsampled coarser level) -> float16 [D, C, g, g]: one fp32 addition and one fp16 rounding, the bits of
    torch's; grids and widths that are no multiple of the 64 x 64 tile, a single token, a sentinel behind the last element."""
    from cryovit_amd.engine import ops

    D = 3
    gen = torch.Generator().manual_seed(g * 1000 + C)
    lat = torch.randn(D * g * g, C, generator=gen)
    n = D * C * g * g
    flat = _sentinel((n + 512,), torch.float16, gpu)
    o16 = flat[:n].view(D, C, g, g)
    lat_d = _nan_rows(lat, D * g * g + 64, C, gpu)
    want = lat.reshape(D, g, g, C).permute(0, 3, 1, 2)
    coarse_d = None
    if with_coarse:
        gc = g // 2
        coarse = torch.randn(D * gc * gc, C, generator=gen)
        coarse_d = _nan_rows(coarse, D * gc * gc + 64, C, gpu)
        want = want + F.interpolate(coarse.reshape(D, gc, gc, C).permute(0, 3, 1, 2), scale_factor=2.0, mode="nearest")
    ops.fpn_level_out(lat_d, coarse_d, o16, slices=D, C=C, grid=g)
    assert torch.equal(_bits(o16.cpu()), _bits(want.half()))
    assert _untouched(flat[n:])


def test_fpn_level_out_refuses_an_odd_grid_with_a_coarse_level(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    D, g, C = 1, 9, 8
    o16 = _sentinel((D, C, g, g), torch.float16, gpu)
    with pytest.raises(_lib.CvxError, match="fpn_level_out"):
        ops.fpn_level_out(torch.zeros(D * g * g, C, device=gpu), torch.zeros(D * 16, C, device=gpu), o16, slices=D, C=C, grid=g)
    torch.cuda.synchronize()
    assert _untouched(o16)


@pytest.mark.parametrize("rows,C", [(1, 8), (37, 144), (300, 1152)])
def test_merge_stream_exact(gpu, rows, C):
    """(hi, lo) bf16 pair -> fp32 x = float(hi) + float(lo), one fp32 addition, bit for bit, for unrelated hi and lo; leading
    dimensions wider than C on both sides.  And merge(split_stream(x)) returns x to within the pair's representation error: hi =
    bf16(x) leaves r = x - hi with |r| <= 2^-8 |x| (half an ulp of 8 significand bits), exact in fp32; lo = bf16(r) leaves at most
    2^-8 |r| <= 2^-16 |x|; the fp32 sum hi + lo rounds once more, 2^-24 |x|."""
    from cryovit_amd.engine import ops

    gen = torch.Generator().manual_seed(rows + C)
    hi, lo = bf(torch.randn(rows, C, generator=gen) * 3), bf(torch.randn(rows, C, generator=gen) * 0.01)
    R = ops.alloc_rows(rows)
    xh, xl = _nan_rows(hi, R, C + 8, gpu), _nan_rows(lo, R, C + 8, gpu)
    x = _sentinel((R, C + 4), torch.float32, gpu)
    ops.merge_stream(xh, xl, x, rows=rows, Cdim=C)
    assert torch.equal(_bits(x[:rows, :C].cpu()), _bits(hi.float() + lo.float()))
    assert _untouched(x[:, C:]) and _untouched(x[rows:])
    x0 = torch.randn(rows, C, generator=gen) * 3 + 0.7
    x0[:, 5] *= 150.0
    sh, sl = _sentinel((R, C + 8), torch.bfloat16, gpu), _sentinel((R, C + 8), torch.bfloat16, gpu)
    ops.split_stream(_nan_rows(x0, R, C + 4, gpu), sh, sl, torch.zeros(R, 2, device=gpu), rows=rows, Cdim=C, eps=1e-6)
    assert _untouched(sh[:, C:]) and _untouched(sl[:, C:]) and _untouched(sh[rows:]) and _untouched(sl[rows:])
    x1 = _sentinel((R, C + 4), torch.float32, gpu)
    ops.merge_stream(sh, sl, x1, rows=rows, Cdim=C)
    err = (x1[:rows, :C].cpu().double() - x0.double()).abs()
    assert bool((err <= (2.0**-16 + 2.0**-24) * x0.double().abs()).all()), float((err / x0.double().abs()).max())


def test_merge_stream_refusals(gpu):
    from cryovit_amd import _lib
    from cryovit_amd.engine import ops

    x = _sentinel((256, 16), torch.float32, gpu)
    h16, h12 = torch.zeros(256, 16, dtype=torch.bfloat16, device=gpu), torch.zeros(256, 12, dtype=torch.bfloat16, device=gpu)
    with pytest.raises(_lib.CvxError, match="merge_stream"):
        ops.merge_stream(h16, h16, x, rows=4, Cdim=12)
    with pytest.raises(_lib.CvxError, match="merge_stream"):
        ops.merge_stream(h12, h12, x, rows=4, Cdim=8)
    torch.cuda.synchronize()
    assert _untouched(x)


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
