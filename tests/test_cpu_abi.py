"""CPU suite, part 2: the C-ABI library builds for gfx950, loads without a GPU and exports every declared symbol;
the product path refuses to run without a device (no CPU fallback)."""

import re
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


def test_header_symbols_all_exported(lib):
    from cryovit_amd import _lib

    header = (ROOT / "include" / "cryovit_hip.h").read_text()
    declared = set(re.findall(r"\b(cvx_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in the header but not exported"


def test_version_and_error_string(lib):
    assert lib.cvx_version() >= 1
    assert isinstance(lib.cvx_last_error(), bytes)


def test_argument_validation_without_gpu(lib):
    # descriptor-less / malformed calls must fail with a message before touching the device
    from cryovit_amd._lib import CvxError, check

    with pytest.raises(CvxError, match="null descriptor"):
        check(lib.cvx_gemm_bf16(None, None), "cvx_gemm_bf16")
    with pytest.raises(CvxError, match="ntp%8"):
        check(lib.cvx_attention_bf16(None, 8, None, None, 8, 1, 1, 10, 10, 64, None), "cvx_attention_bf16")


def test_gemm_refuses_ln_rowstat_without_gpu(lib):
    """cvx_gemm_bf16 turns down a LayerNorm fold it has no kernel for -- fp16 operands, or an epilogue other than BF16 / BF16_GELU /
    SWIGLU / VT -- from the descriptor alone, before any device call (the pointers here are never dereferenced)."""
    from cryovit_amd import _lib

    def desc(epilogue, dtype, ln_rowstat):
        d = _lib.GemmDesc()
        d.epilogue, d.dtype, d.ln_rowstat = epilogue, dtype, ln_rowstat
        d.a = d.w = d.out = d.bias = d.gamma = d.out2 = d.stat_part = d.pos = 16
        d.m, d.n, d.n_pad, d.k_pad, d.lda, d.ldw, d.ldc, d.stat_rows = 256, 128, 128, 64, 64, 64, 128, 512
        return d

    import ctypes

    with pytest.raises(_lib.CvxError, match="ln_rowstat.*bf16 operands"):
        _lib.check(lib.cvx_gemm_bf16(ctypes.byref(desc(_lib.EPI_BF16, _lib.DTYPE_F16, 16)), None), "cvx_gemm_bf16")
    with pytest.raises(_lib.CvxError, match="ln_rowstat.*bf16 operands"):
        _lib.check(lib.cvx_gemm_bf16(ctypes.byref(desc(_lib.EPI_BF16_GELU, _lib.DTYPE_F16, 16)), None), "cvx_gemm_bf16")
    for epi in (_lib.EPI_RESID, _lib.EPI_RESID_HL, _lib.EPI_F32, _lib.EPI_PATCH, _lib.EPI_CONVT):
        with pytest.raises(_lib.CvxError, match="ln_rowstat.*epilogues"):
            _lib.check(lib.cvx_gemm_bf16(ctypes.byref(desc(epi, _lib.DTYPE_BF16, 16)), None), "cvx_gemm_bf16")
    d = desc(_lib.EPI_RESID, _lib.DTYPE_BF16, 16)
    d.m = 0
    assert lib.cvx_gemm_bf16(ctypes.byref(d), None) == 0  # an empty problem stays a no-op


def test_no_cpu_fallback():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from cryovit_amd._lib import CvxError
    from cryovit_amd.engine.vit import VIT_CONFIGS, VitEngine

    with pytest.raises(CvxError):
        VitEngine(VIT_CONFIGS["dinov2_vits14_reg"], {}, "cuda:0")
    from cryovit_amd.engine import ops

    with pytest.raises(CvxError):
        ops.layernorm(torch.zeros(4, 8), torch.ones(8), torch.zeros(8), torch.zeros(4, 8, dtype=torch.bfloat16), 4, 8, 1e-6)


def test_product_never_imports_oracle():
    for f in (ROOT / "cryovit_amd").rglob("*.py"):
        src = f.read_text()
        assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f"{f} imports the oracle"


def test_persistent_gemm_kernels_static_properties():
    """The persistent GEMM tile counts its own vector-memory operations in hand-written vmcnt waits: no spill, an exact
    number of epilogue stores and saddr-form LDS-DMA in the COMPILED gfx950 code are part of its correctness
    (cryovit_amd/check_asm.py; hipcc cross-compiles here without a GPU, ~90 s)."""
    from cryovit_amd import check_asm
    from cryovit_amd.build import CSRC

    gemm_asm = check_asm.compile_asm(CSRC / "gemm.hip")
    report = check_asm.check_gemm256p(gemm_asm)
    assert len(report) >= 10 and any("EpiSwiGLU" in r and "FULL" in r for r in report)
    # the other users of the LDS-DMA helpers: M0 and the DMA only inside inline asm, no scratch
    others = check_asm.check_dma_users(gemm_asm, "gemm.hip")
    for f in check_asm.DMA_SOURCES:
        others += check_asm.check_dma_users(check_asm.compile_asm(CSRC / f), f)
    assert any("k_attentionILi7" in r for r in others) and any("k_conv3_march" in r for r in others)
