#!/usr/bin/env python3
"""Keep at most N points of every sfm/<id>.txt of a dense folder (evenly spaced lines): make_dataset.py --prior writes one point
per 250 pixels, 100 k at 6208x4128, where COLMAP leaves about 10 k per image.
usage: thin_sfm.py FOLDER N"""
import os
import sys

d, n = sys.argv[1], int(sys.argv[2])
for name in sorted(os.listdir(os.path.join(d, "sfm"))):
    fn = os.path.join(d, "sfm", name)
    lines = open(fn).read().splitlines()
    if len(lines) > n:
        step = len(lines) / n
        lines = [lines[int(i * step)] for i in range(n)]
    open(fn, "w").write("\n".join(lines) + "\n")
    print(name, len(lines), "points")
