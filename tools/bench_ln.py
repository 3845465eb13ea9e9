"""Row-normalisation micro-benchmark: LayerNorm at the ViT-g shape (132096 rows x 1536) and the Hiera stage shapes, and at the ViT-g
slice-batch geometry (128 slices x 1032 token rows x 1536) the stream split and the final norm from the bf16 pair with both fp16
outputs: ms and GB/s per launch."""
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from cryovit_amd.engine import ops  # noqa: E402

dev = torch.device("cuda:0")


def timed(name, nbytes, fn):
    for _ in range(3):
        fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(20):
        fn()
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / 20
    print(f"{name}: {ms:.3f} ms  {nbytes / ms / 1e6:.0f} GB/s")


for rows, C, ldo in [(132096, 1536, 1536), (64 * 16384, 144, 192), (64 * 4096, 288, 320), (64 * 1024, 576, 576)]:  # read fp32 + write bf16
    x = torch.randn(rows, C, device=dev)
    w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
    out = torch.zeros(rows, ldo, dtype=torch.bfloat16, device=dev)
    timed(f"layernorm rows {rows} C {C}", rows * C * 6, lambda: ops.layernorm(x, w, b, out, rows, C, 1e-6))

slices, hp, wp, C, tok0 = 128, 32, 32, 1536, 5
ntp = ops.round_up(tok0 + hp * wp, 8)
rows = slices * ntp
x = torch.randn(rows, C, device=dev)
w, b = torch.ones(C, device=dev), torch.zeros(C, device=dev)
xh, xl = torch.zeros(rows, C, dtype=torch.bfloat16, device=dev), torch.zeros(rows, C, dtype=torch.bfloat16, device=dev)
rowstat = torch.zeros(rows, 2, device=dev)
timed(f"split_stream rows {rows} C {C}", rows * C * 8, lambda: ops.split_stream(x, xh, xl, rowstat, rows=rows, Cdim=C, eps=1e-6))  # fp32 in, pair out
del x
f16 = torch.zeros(C, slices, hp, wp, dtype=torch.float16, device=dev)
cl = torch.zeros(slices * hp * wp, C, dtype=torch.float16, device=dev)
timed(f"final_norm_features_hl rows {rows} C {C}", (rows * 4 + 2 * slices * hp * wp * 4) * C,  # the pair read in both phases, two fp16 copies
      lambda: ops.final_norm_features_hl(xh, xl, w, b, 1e-6, slices=slices, ntp=ntp, tok0=tok0, hp=hp, wp=wp, Cdim=C, feats_f16=f16, d_total=slices,
                                         d0=0, feats_cl=cl))
