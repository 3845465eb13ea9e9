"""numpy oracle of the multi-label segmentation overlay (cvx_seg_overlay, cryovit_amd.visualization.segmentations): a
restatement, written from its description, of the arithmetic the reference's ``visualization/segmentations.py:_process_file``
applies to one tomogram.  The reference's own function imports ``cv2`` and ``seaborn`` on its first lines, neither of which is
installed, so it cannot be run here: parity unpinned against the reference's code.

    combined [D,H,W,3] fp32 = 0;  for each label, in order:  combined += stack([seg] * 3) * colour   (fp32 array times a float64
                              colour array -> float64 product, added into the fp32 array: one rounding to fp32 per label)
    combined = clip(combined, 0, 1);  grey = stack([clip(data, 0, 1)] * 3)
    right = where(combined > threshold, combined, grey)        (per channel; a Python float threshold compares as fp32)
    frames = (concatenate([grey, right], axis=2) * 255).astype(uint8)                      [D, H, 2W, 3]
"""

import numpy as np

PALETTE = {
    "mito": (0x4C / 255, 0x72 / 255, 0xB0 / 255),
    "cristae": (0xDD / 255, 0x84 / 255, 0x52 / 255),
    "microtubule": (0x55 / 255, 0xA8 / 255, 0x68 / 255),
    "granule": (0xC4 / 255, 0x4E / 255, 0x52 / 255),
}


def overlay_frames(data, volumes, colours, threshold=0.5):
    """uint8 [D, H, 2W, 3]: ``data`` [D, H, W] (any real dtype), ``volumes`` a list of [D, H, W] label volumes (probabilities or
    masks), ``colours`` one RGB triple of Python floats per volume, ``threshold`` a Python float."""
    data = np.asarray(data).astype(np.float32)
    combined = np.zeros((*data.shape, 3), dtype=np.float32)
    for seg, colour in zip(volumes, colours, strict=True):
        seg = np.asarray(seg).astype(np.float32)
        assert seg.shape == data.shape, (seg.shape, data.shape)
        tint = np.array(colour, dtype=np.float64).reshape(1, 1, 1, 3)
        combined += np.stack([seg, seg, seg], axis=-1) * tint
    combined = np.clip(combined, 0, 1)
    grey = np.clip(data, 0, 1)
    grey = np.stack([grey, grey, grey], axis=-1)
    right = np.where(combined > float(threshold), combined, grey)
    both = np.concatenate([grey, right], axis=2)
    assert both.dtype == np.float32
    return (both * 255).astype(np.uint8)
