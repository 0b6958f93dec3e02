"""Train a DBoW2 ORB vocabulary from the frames of an rgbd_mmt sequence directory (image/%06d.png,
settings.yaml) on the GPU: ORB extraction, TemplatedVocabulary::create and saveToTextFile through
libmmt (mmt_orb_extract, mmt_train_vocabulary, mmt_save_vocabulary).

Usage: python tools/train_vocabulary.py SEQ_DIR OUT.txt [-k 10] [-L 6] [--step 1] [--seed 0]
"""
import argparse
import glob
import os
import sys

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import multimot_track_amd as M  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("seq")
    ap.add_argument("out")
    ap.add_argument("-k", type=int, default=10)
    ap.add_argument("-L", type=int, default=6)
    ap.add_argument("--step", type=int, default=1, help="take every step-th frame")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--features", type=int, default=2000, help="ORBextractor.nFeatures")
    a = ap.parse_args()
    files = sorted(glob.glob(os.path.join(a.seq, "image", "*.png")))[::a.step]
    ctx, descs = None, []
    for f in files:
        # imread's BGR bytes through cvtColor(RGB2GRAY), as Tracking::GrabImageRGBD with Camera.RGB: 1
        c = np.asarray(Image.open(f).convert("RGB"), np.int32)[:, :, ::-1]
        gray = ((c[:, :, 0] * 4899 + c[:, :, 1] * 9617 + c[:, :, 2] * 1868 + 8192) >> 14).astype(np.uint8)
        if ctx is None:
            ctx = M.Context(M.kitti03_config(gray.shape[1], gray.shape[0], a.features))
        descs.append(ctx.orb_extract(gray)[1])
    st = ctx.train_vocabulary(descs, a.k, a.L, seed=a.seed)
    ctx.save_vocabulary(a.out)
    print("%d frames, %d descriptors -> %s: %s" % (len(files), sum(map(len, descs)), a.out, st))
    ctx.close()


if __name__ == "__main__":
    main()
