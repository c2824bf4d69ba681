#!/usr/bin/env python3
"""Score a list of still-image pairs in batches on the GPU (fvvdp.predict_image_pairs).

    python examples/ex_image_folder.py TEST_DIR REF_DIR      # pairs matched by file name (PNG / JPEG via Pillow, .npy)
    python examples/ex_image_folder.py                       # synthetic pairs of three sizes

Pairs of one size and sample type are evaluated together: one ingest launch, one launch per pyramid level (pair) and one pooling
launch per batch of up to 128 pairs, instead of one predict() call per pair.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fovvideovdp_amd as pyfvvdp


def load(path):
    if path.endswith(".npy"):
        return np.load(path)
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def synthetic_pairs():
    rs = np.random.RandomState(0)
    pairs, names = [], []
    for (H, W) in ((512, 512), (720, 1280), (300, 401)):
        for k in range(4):
            ref = (rs.rand(H, W, 3) * 255).astype(np.uint8)
            noise = rs.randn(H, W, 3) * (2 + 4 * k)
            test = np.clip(ref + noise, 0, 255).astype(np.uint8)
            pairs.append((test, ref))
            names.append("synthetic_%dx%d_noise%d" % (W, H, k))
    return pairs, names


def main():
    if len(sys.argv) == 3:
        tdir, rdir = sys.argv[1], sys.argv[2]
        names = sorted(f for f in os.listdir(tdir) if os.path.isfile(os.path.join(rdir, f)))
        pairs = [(load(os.path.join(tdir, f)), load(os.path.join(rdir, f))) for f in names]
    else:
        pairs, names = synthetic_pairs()
    metric = pyfvvdp.fvvdp(display_name="standard_fhd")
    results = metric.predict_image_pairs(pairs, dim_order="HWC")
    for name, (q, stats) in zip(names, results):
        print("%-40s %6.3f JOD  (%dx%d)" % (name, float(q), stats["width"], stats["height"]))


if __name__ == "__main__":
    main()
