"""The named inputs of the TGA encoder tests: rows whose packets are known, contents that exercise the packet chain, and the batch
that the GPU test encodes in one call."""
import numpy as np

# one row of l8 values -> the reference's packets (R<n>: run-length packet of n pixels, raw<n>: raw packet of n)
KNOWN_ROWS = [
    ("abb_x4", [0, 1, 1] * 4, ["raw2", "raw3", "raw3", "raw3", "raw1"]),
    ("run_129_then_one", [5] * 129 + [6], ["R128", "raw2"]),
    ("run_257", [5] * 257, ["R128", "R128", "raw1"]),
    ("all_different_130", list(range(130)), ["raw128", "raw2"]),
    ("abbc", [0, 1, 1, 2], ["raw2", "raw2"]),
    ("raw_128_then_run_5", list(range(128)) + [200] * 5, ["raw128", "R5"]),
    ("raw_127_then_run_5", list(range(127)) + [200] * 5, ["raw128", "R4"]),
]

WIDTHS = [1, 2, 3, 127, 128, 129, 130, 255, 256, 257, 258]
CONTENTS = ["equal", "different", "abb", "stretch126", "stretch127", "stretch128", "alphabet", "alpha_only", "grey_only"]


def _different(n, rng):
    """n values, neighbours never equal"""
    v = rng.integers(0, 255, n).astype(np.int64)
    for i in range(1, n):
        if v[i] == v[i - 1]:
            v[i] = (v[i] + 1) % 255
    return v


def content(kind, w, h, comp, seed):
    """(h, w, comp) uint8.  Kinds that are about a channel the type does not have fall back to the random alphabet."""
    rng = np.random.default_rng(seed)
    img = np.zeros((h, w, comp), np.uint8)
    for y in range(h):
        if kind == "equal":
            key = np.full(w, int(rng.integers(0, 256)))
        elif kind == "different":
            key = _different(w, rng)
        elif kind == "abb":
            key = np.resize(np.array([7, 9, 9]), w + y)[y:]                   # the phase moves with the row
        elif kind.startswith("stretch"):
            n = int(kind[7:]) - (y % 2)                                      # a raw stretch, then runs of 2, 3 and 129, repeated
            unit = np.concatenate([_different(n, rng) % 200, [250, 250], [251] * 3, [252] * 129])
            key = np.resize(unit, w)
        else:
            key = rng.integers(0, int(rng.integers(2, 5)), w)
        key = np.asarray(key, np.int64)
        for c in range(comp):
            img[y, :, c] = (key * (c + 1) + 3 * c) % 256
        if kind == "alpha_only" and comp in (2, 4):                          # equal in colour, different in alpha
            img[y, :, : comp - 1] = 77
            img[y, :, comp - 1] = _different(w, rng)
        if kind == "grey_only" and comp == 2:                                # equal in alpha, different in grey
            img[y, :, 0] = _different(w, rng)
            img[y, :, 1] = 200
    return img


def matrix_images(extra_widths=()):
    """the images of the one batched call: every source type x every width, heights 1..5, the contents in turn -> [(name, img)]"""
    out = []
    k = 0
    for comp in (1, 2, 3, 4):
        for w in list(WIDTHS) + [int(x) for x in extra_widths]:
            for kind in CONTENTS:
                if kind == "alpha_only" and comp not in (2, 4):
                    continue
                if kind == "grey_only" and comp != 2:
                    continue
                if kind.startswith("stretch") and w < 127:
                    continue
                h = 1 + k % 5
                out.append((f"c{comp}_w{w}_h{h}_{kind}", content(kind, w, h, comp, 1000 + k)))
                k += 1
    return out


def random_images(n, seed=0, max_w=399):
    """small alphabets so that runs abound: 1-4 channels, widths 1..max_w, heights 1..4"""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        comp, w, h = int(rng.integers(1, 5)), int(rng.integers(1, max_w + 1)), int(rng.integers(1, 5))
        a = int(rng.integers(2, 5))
        img = rng.integers(0, a, (h, w, comp)).astype(np.uint8)
        if i % 3 == 0:                                                       # long runs too
            img = np.repeat(img, int(rng.integers(2, 140)), axis=1)[:, :w]
        if i % 4 == 1:                                                       # one key for all channels: whole-pixel runs
            img = np.repeat(img[:, :, :1], comp, axis=2)
        out.append((f"random{i}_c{comp}_{w}x{h}", np.ascontiguousarray(img)))
    return out
