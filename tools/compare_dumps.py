#!/usr/bin/env python
"""Compare two `bench.py --dump-outputs` directories file by file (CPU only, reads the .npy files).

For every .npy file in either directory prints whether the two arrays are bit-equal, the largest absolute difference and the
fraction of elements that differ.  Exit status 0 only when every file is present in both directories and bit-equal.
usage: compare_dumps.py DIR_A DIR_B"""
import os
import sys

import numpy as np


def compare(a_dir, b_dir, out=sys.stdout):
    """-> True when both directories hold the same .npy files with bit-equal contents."""
    names = sorted({f for d in (a_dir, b_dir) for f in os.listdir(d) if f.endswith('.npy')})
    if not names:
        print(f'no .npy files in {a_dir} or {b_dir}', file=out)
        return False
    ok = True
    for name in names:
        pa, pb = os.path.join(a_dir, name), os.path.join(b_dir, name)
        missing = [d for d, p in ((a_dir, pa), (b_dir, pb)) if not os.path.isfile(p)]
        if missing:
            print(f'{name:36s} MISSING in {", ".join(missing)}', file=out)
            ok = False
            continue
        a, b = np.load(pa), np.load(pb)
        if a.shape != b.shape or a.dtype != b.dtype:
            print(f'{name:36s} DIFFERENT shape / dtype: {a.shape} {a.dtype} vs {b.shape} {b.dtype}', file=out)
            ok = False
            continue
        # bit-equal: the raw bytes (NaNs with equal payloads count as equal, -0.0 and 0.0 do not)
        if a.size:
            ra, rb = (np.ascontiguousarray(x).reshape(-1).view(np.uint8).reshape(a.size, -1) for x in (a, b))
            ne = (ra != rb).any(axis=1)
        else:
            ne = np.zeros(0, bool)
        equal = not ne.any()
        if a.size and np.issubdtype(a.dtype, np.number):
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            maxabs = float(np.nanmax(d)) if not np.all(np.isnan(d)) else float('nan')
        else:
            maxabs = 0.0
        frac = float(ne.mean()) if a.size else 0.0
        print(f'{name:36s} {"bit-equal" if equal else "DIFFERENT"}  max|a-b| = {maxabs:.3e}  differing = {frac:.3e} '
              f'({int(ne.sum())} of {a.size})', file=out)
        ok &= equal
    return ok


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        print(__doc__.strip().splitlines()[-1], file=sys.stderr)
        return 2
    ok = compare(*argv)
    print('all files bit-equal' if ok else 'directories differ')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
