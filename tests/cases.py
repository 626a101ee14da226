"""Shared parity cases: shapes, flag combinations and tile calls (used by the golden
generator, the CPU tests and the GPU tests)."""
import hashlib
from pathlib import Path

import numpy as np

FLAG_COMBOS = {
    "none": dict(),
    "specified": dict(specified=True),
    "specified_periodic_x": dict(specified=True, periodic_x=True),
    "nested": dict(nested=True),
}

# name -> (NI, NK, NJ, tile override or None)
# tile override = dict(its=, ite=, jts=, jte=) relative to the single-patch domain
SHAPES = {
    "16x8x16": (16, 8, 16, None),
    "64x40x64": (64, 40, 64, None),               # BASELINE.json configs[0]
    "37x5x11_ragged": (37, 5, 11, None),          # nothing a multiple of anything
    "130x3x7_tile": (130, 3, 7, dict(its=60, ite=70, jts=3, jte=5)),   # interior tile call
    "70x1x9_onelevel": (70, 1, 9, None),          # k_end = 1: recurrence loop is empty
    "5x60x4_thin": (5, 60, 4, None),
}


GOLDEN = Path(__file__).resolve().parent / "golden"
# the reference's full output arrays (tests/golden/make_golden.py), in two files: one would pass 1 MiB
GOLDEN_SMALL = {"golden_small.npz": ("16x8x16", "37x5x11_ragged"), "golden_small_shapes.npz": ("130x3x7_tile", "70x1x9_onelevel")}


def load_small() -> dict:
    """Every array of GOLDEN_SMALL's files, keyed '<shape>/<flags>/<dtype>/<output>'."""
    out = {}
    for name in GOLDEN_SMALL:
        with np.load(GOLDEN / name) as z:
            out.update({k: z[k] for k in z.files})
    return out


def digest(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a).view(np.uint8).tobytes()).hexdigest()


def digest_canonical_nan(a) -> str:
    """digest() after mapping every NaN to the positive quiet NaN without payload: which NaN a platform generates or propagates
    is not part of the comparison (tests/special_values.py)."""
    a = np.ascontiguousarray(a).copy()
    a[np.isnan(a)] = np.nan
    return digest(a)


def make_case(pkg, shape_name, flag_name, dtype, seed=12345, aligned=False):
    ni, nk, nj, tile = SHAPES[shape_name]
    b = pkg.synth.domain_bounds(ni, nk, nj, aligned=aligned)
    if tile:
        b = b.replace(**tile)
    return pkg.synth.make_patch(b, pkg.GridConfig(**FLAG_COMBOS[flag_name]), dtype=dtype, seed=seed,
                                global_dims=(ni, nk, nj))


EXTRA_TRIALS = 6          # extra seeds / shapes checked against the reference (tests/golden/extra_reference_digests.json)


def extra_case(pkg, trial, dtype):
    """Extra case `trial`: a random shape of 3..39 cells per axis (unpadded and padded rows in turn), a flag combination and a
    seed of its own -- the same case on every host."""
    rng = np.random.default_rng(0)
    shapes = [tuple(int(x) for x in rng.integers(3, 40, 3)) for _ in range(EXTRA_TRIALS)]
    ni, nk, nj = shapes[trial]
    b = pkg.synth.domain_bounds(ni, nk, nj, aligned=bool(trial % 2))
    flags = list(FLAG_COMBOS.values())[trial % 4]
    return pkg.synth.make_patch(b, pkg.GridConfig(**flags), dtype=dtype, seed=1000 + trial)
