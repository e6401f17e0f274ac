"""The inputs the KDE tests share (tests/test_scanpath_kde_cpu.py measures the summation-order spread on them, test_scanpath_kde_gpu.py
runs the device on them): built once per map, never changed.

Six images under shuffled, non-contiguous group ids (ids 0, 1, 2, .. 20 that hold no scanpath lie between them):
  11  one scanpath (no other scanpath: others = 0, NaN);          3  two scanpaths: the special fixations and their duplicates;
  20  63 fixations in all (20 + 20 + 23);   7  64 in all (30 + 34);   5  65 in all (64 + 1 + a scanpath of 0 fixations);
  14  big: 40 scanpaths of 64 fixations (2560 points, more than any one tile); otherwise 3 scanpaths of 20.
The scanpaths come interleaved (a fixed permutation), with a duration column.  The special fixations, each a query and a source (image 3
has two scanpaths): on a cell border, at a corner of four cells, at the last pixel, at nextafter(w, 0), at x = w, negative, NaN, inf,
and one that the other scanpath repeats exactly at the same step.
The fixations of an image scatter around its three hot spots (sd 0.07 of the side), so that every leave-out score has an interior best
bandwidth.  Random coordinates keep 0.03 .. 0.05 px away from being that near a cell centre on either axis, so that at bandwidth 1e-3 no exponent
argument lies between -800 and -700 (the tests assert it on the restatement)."""
import numpy as np

MAPS = {(1, 1): (24.0, 32.0), (1, 2): (2.0, 4.0), (3, 5): (30.0, 50.0), (8, 8): (37.0, 53.0), (5, 13): (240.0, 320.0),
        (30, 40): (240.0, 320.0), (32, 64): (240.5, 320.25)}
BIG = ((30, 40),)                             # the maps whose image 14 holds 2560 fixations
IDS = dict(one=11, two=3, n63=20, n64=7, n65=5, many=14)
_CASES = {}


def bandwidths(shape):
    """1e-3 (one-hot), 0.5, one cell pitch, 45.3, 1e6 (uniform)"""
    return [1e-3, 0.5, MAPS[shape][1] / shape[1], 45.3, 1e6]


BW0 = (1e-3, 45.3, 1e6)                       # the bandwidths of the uniform_mix = 0 runs (module docstring)


def _coords(g, spots, length, cells):
    """one coordinate around each of the given hot spots (sd 0.07 of the side), inside the frame"""
    out = np.empty(len(spots))
    for i, spot in enumerate(spots):
        while True:
            v = g.normal(spot, 0.07 * length)
            d = np.abs(v - (np.arange(cells) + 0.5) * length / cells).min()
            if 0.0 <= v < length and not 0.03 < d < 0.05:
                break
        out[i] = v
    return out


def case(shape, big=None):
    """(scanpaths, image_groups, frame)"""
    big = shape in BIG if big is None else big
    if (shape, big) in _CASES:
        return _CASES[shape, big]
    (Hm, Wm), (h, w) = shape, MAPS[shape]
    g = np.random.default_rng(77 * Hm + Wm)

    spots = {name: g.uniform(0.15, 0.85, (3, 2)) * (w, h) for name in IDS}      # people look at an image's three hot spots

    def path(n, name):
        at = spots[name][g.integers(0, 3, n)]
        return np.stack([_coords(g, at[:, 0], w, Wm), _coords(g, at[:, 1], h, Hm), g.uniform(0.05, 0.8, n)], 1)

    special = [(min(3, Wm - 1) * w / Wm, h / 3), (min(2, Wm - 1) * w / Wm, min(2, Hm - 1) * h / Hm), (w - 1.0, h - 1.0),
               (np.nextafter(w, 0), np.nextafter(h, 0)), (w, h / 2), (w / 2, -0.25), (np.nan, h / 2), (w / 3, np.inf)]
    a = path(len(special) + 1, "two")
    a[:len(special), :2] = special
    b = path(12, "two")
    b[len(special), :2] = a[len(special), :2]                    # two identical fixations in different scanpaths, at the same step
    b[2, :2] = a[0, :2]                                          # and the border fixation again at another step
    paths = [(a, "two"), (b, "two"), (np.zeros((0, 3)), "n65")]
    paths += [(path(n, name), name) for n, name in ((5, "one"), (20, "n63"), (20, "n63"), (23, "n63"), (30, "n64"), (34, "n64"),
                                                    (64, "n65"), (1, "n65"))]
    paths += [(path(64, "many"), "many") for _ in range(40)] if big else [(path(20, "many"), "many") for _ in range(3)]
    perm = g.permutation(len(paths))
    out = ([paths[i][0] for i in perm], [IDS[paths[i][1]] for i in perm], (h, w))
    _CASES[shape, big] = out
    return out
