"""Generates tests/golden/jet_lut.npz: matplotlib's `jet` colour map as a 256 x 3 uint8 table (the entries of its
256-entry lookup table, converted to bytes by matplotlib itself).  monogs_amd.viewer.JET_LUT must equal it byte for
byte (tests/test_cpu_viewer.py); the tests do not import matplotlib.

Run from the repository root:  python tests/golden/make_jet_lut.py        (matplotlib 3.10)
`--hex` also prints the table as the hex string viewer.py embeds."""
import os
import sys

import numpy as np


def jet_table() -> np.ndarray:
    import matplotlib
    cmap = matplotlib.colormaps["jet"].resampled(256)
    lut = cmap(np.arange(256), bytes=True)[:, :3]
    return np.ascontiguousarray(lut, dtype=np.uint8)


if __name__ == "__main__":
    import matplotlib
    lut = jet_table()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "jet_lut.npz")
    np.savez_compressed(out, lut=lut, matplotlib_version=np.array(matplotlib.__version__))
    print(f"wrote {out}: {lut.nbytes} bytes, first {lut[0].tolist()}, middle {lut[128].tolist()}, last {lut[255].tolist()}")
    if "--hex" in sys.argv:
        h = lut.tobytes().hex()
        for i in range(0, len(h), 96):
            print(f'    "{h[i:i + 96]}"')
