"""Inputs without the generator's symmetries, layered over a patch in the tests only (pure numpy).

The generator (include/amt_synth.h) makes the vertical metrics a function of the level alone with a short period: dnw and
rdnw repeat every 8 levels and are mirror-symmetric, fnm and fnp every 16, and fnp == 1 - fnm exactly.  Every patch also
carries the same four scalars, with a power-of-two dts.  A kernel that reads another wave's metrics, reverses a chunk's
level order, rebuilds fnp from fnm, forms an FMA in mu + dts*(...) or steps with stale scalars passes every test on those
inputs.  Here:

* ``wrf_levels``: the metrics of a seeded, irregularly stretched eta column, computed in the array's own precision the way
  WRF's initialisation computes them (dnw, rdnw, dn, fnm, fnp); every memory level the routine does not read holds a distinct
  finite value of its own, so reading a wrong level changes the answer.
* ``apply``: writes them into a host patch (numpy) or a device patch (torch, ``native_domain=True`` patches included: their
  tensors view the handle's memory) and sets the patch's scalars, rounded once to the patch's precision so that every path
  (the oracle, the C-ABI's T arguments, ``amt_domain_set_scalars``' doubles) receives the same value.
* ``SCALAR_SETS``: scalars with long mantissas (``dts`` as dts_rk of an RK stage), rdx != rdy but for one dx == dy set.
"""
from __future__ import annotations

import numpy as np

RANK1 = ("dnw", "fnm", "fnp", "rdnw")

SCALAR_SETS = {
    "rk3_dx12km": dict(rdx=1.0 / 12000.0, rdy=1.0 / 11000.0, dts=20.0 / 3.0, epssm=0.1),
    "rk2_dx3km": dict(rdx=1.0 / 3000.0, rdy=1.0 / 3000.0, dts=10.0 / 3.0, epssm=0.1),        # WRF's common dx == dy
    "rk1_dx1km": dict(rdx=1.0 / 1000.0, rdy=1.0 / 1333.0, dts=0.3, epssm=0.35),
    "nest_dx333m": dict(rdx=3.0 / 1000.0, rdy=3.0 / 1001.0, dts=1.1, epssm=1.0),
}


def rounded_scalars(scalars: dict, dtype) -> dict:
    """The scalars as the patch's precision holds them (as Python floats)."""
    t = np.dtype(dtype).type
    return {k: float(t(v)) for k, v in scalars.items()}


def _column(nk: int, rng) -> np.ndarray:
    """znw(1..nk+1) in float64: 1 at the surface, 0 at the top, thin layers near the ground stretching upwards, each layer
    thickness perturbed by a random factor."""
    x = np.arange(nk, dtype=np.float64) / max(nk - 1, 1)
    thick = (0.35 + x ** 1.6) * rng.uniform(0.7, 1.3, nk)
    znw = np.empty(nk + 1)
    znw[0] = 1.0
    znw[1:] = 1.0 - np.cumsum(thick) / thick.sum()
    znw[-1] = 0.0
    return znw


def _metrics(znw, t):
    """dnw(1..nk), fnm, fnp, dn (index k-1 holds level k; level 1 of fnm, fnp, dn is 0) in the precision of ``znw``."""
    nk = len(znw) - 1
    dnw = znw[1:] - znw[:-1]                                # dnw(k) = znw(k+1) - znw(k)
    dn = np.zeros(nk, znw.dtype)
    fnm = np.zeros(nk, znw.dtype)
    fnp = np.zeros(nk, znw.dtype)
    if nk > 1:
        dn[1:] = t(0.5) * (dnw[1:] + dnw[:-1])              # dn(k) = 0.5*(dnw(k) + dnw(k-1))
        fnm[1:] = t(0.5) * dnw[1:] / dn[1:]                 # fnm(k) = 0.5*dnw(k)/dn(k)
        fnp[1:] = t(0.5) * dnw[:-1] / dn[1:]                # fnp(k) = 0.5*dnw(k-1)/dn(k)
    return dnw, fnm, fnp, dn


def wrf_levels(nk: int, dtype, seed: int, kms: int = 1, kme: int | None = None) -> dict:
    """dnw, fnm, fnp, rdnw of an ``nk``-layer column (kde = nk + 1) as arrays over the memory levels kms..kme (default
    1..kde).  Column levels the routine reads: dnw, rdnw at 1..nk; fnm, fnp at 2..nk.  Every other memory level holds a
    distinct finite value that no column level has."""
    dt = np.dtype(dtype)
    t = dt.type
    kde = nk + 1
    kme = kde if kme is None else kme
    if kms > 1 or kme < kde:
        raise ValueError("memory levels must cover 1..kde")
    rng = np.random.default_rng([int(seed), int(nk), dt.itemsize])
    for _ in range(100):
        znw = _column(nk, rng).astype(dt)
        # fl(fnm + fnp) rounds to 1 on almost every level, but fnp and fl(1 - fnm) differ on about a third of them: move
        # the top of layer k (znw(k+1), which only levels k..k+2 read) by a few ulps until they differ at level k too
        for k in range(2, nk):
            for _ in range(40):
                dnw, fnm, fnp, _dn = _metrics(znw, t)
                if fnp[k - 1] != t(1) - fnm[k - 1]:
                    break
                znw[k] = znw[k] * t(1 + rng.uniform(-64, 64) * np.finfo(dt).eps)
        dnw, fnm, fnp, _dn = _metrics(znw, t)
        rdnw = (t(1) / dnw).astype(dt)
        if (len(set(dnw.tolist())) == nk and len(set(fnm[1:].tolist())) == nk - 1 and (dnw < 0).all()):
            break
    else:
        raise RuntimeError("no column with distinct levels")
    n = kme - kms + 1
    col = slice(1 - kms, 1 - kms + nk)                          # memory index of levels 1..nk
    out = {}
    # filler of the levels the routine never reads: distinct, finite, of the column's magnitude, and different from every
    # value of the column (dnw < 0 in the column, > 0 here; fnm, fnp in (0, 1) there, in (1.25, 1.75) here)
    m = np.arange(n, dtype=np.float64)
    fill = {"dnw": 0.013 + 0.0007 * m, "rdnw": 61.0 + 1.37 * m, "fnm": 1.25 + 0.5 * (m + 0.5) / n, "fnp": 1.75 - 0.5 * (m + 0.25) / n}
    for name, vals in (("dnw", dnw), ("fnm", fnm), ("fnp", fnp), ("rdnw", rdnw)):
        a = fill[name].astype(dt)
        a[col] = vals
        out[name] = a
    for name in ("fnm", "fnp"):                                 # level 1 of fnm / fnp is not read either
        out[name][1 - kms] = fill[name][1 - kms].astype(dt)
    return out


def levels_for(patch, seed: int) -> dict:
    """wrf_levels over the memory levels of ``patch``, column height kde - 1."""
    b = patch.bounds
    dt = patch.arrays["dnw"].dtype
    dtype = np.float64 if "64" in str(dt) else np.float32
    return wrf_levels(b.kde - 1, dtype, seed, b.kms, b.kme)


def apply(patch, levels: dict | None, scalars: dict | None):
    """Overwrite the four rank-1 arrays of ``patch`` with ``levels`` (host: numpy; device: torch tensors, written in place,
    so a ``native_domain=True`` patch's handle sees them) and set its scalars, rounded to its precision.  Returns patch."""
    a = patch.arrays
    is_torch = hasattr(a["dnw"], "is_cuda")
    dtype = np.float64 if "64" in str(a["dnw"].dtype) else np.float32
    if levels is not None:
        for name in RANK1:
            v = np.asarray(levels[name], dtype=dtype)
            if tuple(v.shape) != tuple(a[name].shape):
                raise ValueError(f"{name}: {v.shape} does not fit {tuple(a[name].shape)}")
            if is_torch:
                import torch
                a[name].copy_(torch.from_numpy(v))
            else:
                a[name][...] = v
    if scalars is not None:
        r = rounded_scalars(scalars, dtype)
        patch.rdx, patch.rdy, patch.dts, patch.epssm = r["rdx"], r["rdy"], r["dts"], r["epssm"]
    return patch


def significant_bits(x: float) -> int:
    """Bits of the significand of ``x`` up to its last set bit (1 for a power of two)."""
    m, _ = np.frexp(abs(float(x)))
    n = 0
    while m != np.floor(m):
        m *= 2.0
        n += 1
    return max(n, 1)


# ---------------------------------------------------------------------------------------------
# Reference-anchored cases (tests/golden/hard_inputs_digests.json, written by tests/golden/make_golden.py): the patches of
# cases.SHAPES plus one tall sub-tile, with wrf_levels and every scalar set.
# ---------------------------------------------------------------------------------------------
LEVEL_SEED = 2027
EXTRA_SHAPES = {"48x41x20_tile": (48, 41, 20, dict(its=9, ite=37, jts=4, jte=15))}     # 41 levels on an interior sub-tile


def hard_shapes() -> dict:
    import cases
    return dict(cases.SHAPES, **EXTRA_SHAPES)


def hard_case(pkg, shape_name, flag_name, dtype, set_name, seed=12345):
    """The patch of ``shape_name`` (cases.make_case's inputs) with wrf_levels(LEVEL_SEED) and SCALAR_SETS[set_name]."""
    import cases
    ni, nk, nj, tile = hard_shapes()[shape_name]
    b = pkg.synth.domain_bounds(ni, nk, nj)
    if tile:
        b = b.replace(**tile)
    p = pkg.synth.make_patch(b, pkg.GridConfig(**cases.FLAG_COMBOS[flag_name]), dtype=dtype, seed=seed, global_dims=(ni, nk, nj))
    return apply(p, levels_for(p, LEVEL_SEED), SCALAR_SETS[set_name])


def hard_keys():
    import cases
    return [f"{shape}/{flag}/{np.dtype(dt).name}/{s}" for shape in hard_shapes() for flag in cases.FLAG_COMBOS
            for dt in (np.float32, np.float64) for s in SCALAR_SETS]
