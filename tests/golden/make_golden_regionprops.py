"""Golden vectors that pin the measure stage's conventions to scikit-image (0.18.3, the version the other skimage
fixtures were made with; run under the interpreter that has it):

    python3.9 tests/golden/make_golden_regionprops.py

`skimage.measure.regionprops_table` on three small seeded label maps with a uint16 intensity image; inputs and
outputs are stored in g13_regionprops.npz.  Uses numpy and scikit-image only.
"""

import os

import numpy as np
from skimage.measure import regionprops_table

HERE = os.path.dirname(os.path.abspath(__file__))
PROPERTIES = ("label", "area", "bbox", "centroid", "inertia_tensor_eigvals", "equivalent_diameter", "mean_intensity",
              "min_intensity", "max_intensity")


def blobs(shape, n, rng):
    """n ellipsoids at random places, later ones over earlier ones"""
    lab = np.zeros(shape, dtype=np.int32)
    grid = np.indices(shape).astype(np.float64)
    for i in range(1, n + 1):
        centre = [rng.uniform(0, s) for s in shape]
        radius = [rng.uniform(1.5, max(2.0, s / 4)) for s in shape]
        d = sum(((g - c) / r) ** 2 for g, c, r in zip(grid, centre, radius))
        lab[d <= 1.0] = i
    return lab


def main():
    rng = np.random.RandomState(13)
    cases = {}
    cases["2d"] = blobs((40, 52), 14, rng)
    edge = np.zeros((23, 31), dtype=np.int32)
    edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = 3          # one object touching all four borders
    edge[11, 4:27] = 3
    edge[0:12, 4] = 3
    edge[5, 9] = 7                                                    # a one-pixel object
    edge[14:20, 8:19] = 2
    edge[16:18, 10:13] = 0                                            # with a hole
    cases["2d_edge"] = edge
    cases["3d"] = blobs((8, 12, 16), 9, rng)
    out = {}
    for name, lab in cases.items():
        raw = rng.randint(0, 65536, size=lab.shape).astype(np.uint16)
        out[f"{name}/labels"] = lab
        out[f"{name}/raw"] = raw
        table = regionprops_table(lab, intensity_image=raw, properties=PROPERTIES)
        for key, value in table.items():
            out[f"{name}/{key}"] = np.asarray(value)
    np.savez_compressed(os.path.join(HERE, "g13_regionprops.npz"), **out)
    import skimage
    print("written g13_regionprops.npz with scikit-image", skimage.__version__, sorted(k for k in out if k.startswith("3d/")))


if __name__ == "__main__":
    main()
