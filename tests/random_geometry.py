"""TEST INFRASTRUCTURE: seeded random geometries for the streaming kernels, the ensemble launch and the handles -- the cases of
tests/test_gpu_12b_random_geometry.py, and without a GPU the proof that those cases have teeth
(tests/test_random_geometry_cpu.py).  No device call in this file.

``draw(rng, family)`` gives one ``Case``: bounds, flags, dtype, members and the family's own parameters; ``cases(family)`` the
seeded campaign of a family.  ``run(case, ops)`` is the family's SCRIPT -- it makes the inputs of the case (random finite values
where the contract reads, NaN with a payload of its own everywhere else) and plays the family's calls through ``ops``, an object
with one method per library call that works IN PLACE on numpy arrays -- and returns the arrays of the call, whole, inputs
included, after every call.  ``RefOps`` are the numpy references of the tree; the GPU campaign plays the same script through
ops that upload, call the library and download; the mutants of the CPU test play it through deliberately wrong references.
``first_difference`` is the one comparison all of them go through: bytes, whole arrays.  The sweep families (ensemble, handles)
start from synth.make_patch, which fills every cell: there the poison goes over it, outside the read mask of advance_mu_t
(tests/special_values.py) and, on the handles, outside the union of what the calls of the composition read.

Sizes.  Draws are small: the smallest shapes at which these kernels can still go wrong.  About one draw in twenty is
mid-sized, so that a launch needs more than one pass of its grid.  The launchers' own block rules:
  amt_sumflux.hip, amt_stage.hip, amt_bdy.hip, amt_halo.hip:  blocks = min((total + 255) / 256, 1024) of 256 threads,
      total = runs * 16-byte chunks per run of a job: the grid-stride loop iterates when total > 1024 * 256 = 262144
  amt_moments.hip:  blocks = min((total + 255) / 256, 2048): total > 2048 * 256 = 524288
  amt_diag.hip:  a workgroup takes groups of 256 >> shift runs, nwg = min(ceil(groups / 4), 2048), lanes along a run 1 << shift
      with shift <= 8: the group loop iterates when groups > nwg, the chunk loop when a run has more than 256 chunks
  the march and column kernels launch one workgroup per tile of a member and have no such loop: a mid-sized draw there has
      several i tiles and several row blocks per member.
What the mid-sized draws do NOT reach: with both cyclic axes only the row jobs of the refresh pass 262144 items (the column
jobs would need as many rows as well); a mid-sized draw of the handles family is sized for the handle's stage and sumflux
launches (both on in such a draw), its zone update and cyclic refresh stay inside one pass -- those two go round their grids
in their own families only.
"""
from __future__ import annotations

import os
from contextlib import contextmanager
from dataclasses import dataclass, field

import numpy as np

import cyclic_ref as CR
import diag_ref as DR
import moments_ref as MR
import specbdy_ref as SB
import stage_ref as ST
import sumflux_ref as SF

FAMILIES = ("ensemble", "cyclic", "spec_bdy", "sumflux", "stage", "moments", "diag", "handles")
DEFAULT_SEED = 20261020
SEED = int(os.environ.get("AMT_GEOM_SEED", DEFAULT_SEED))
DEFAULT_CASES = {"ensemble": 200, "cyclic": 200, "spec_bdy": 200, "sumflux": 200, "stage": 200, "moments": 200, "diag": 200,
                 "handles": 40}
N_CASES = {f: int(os.environ.get("AMT_GEOM_CASES", n)) for f, n in DEFAULT_CASES.items()}

F64, F32 = np.float64, np.float32
NI_SET = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 64, 65)
NK_SET = (1, 2, 3, 4, 5, 7)
KMS_SET = (1, 0, -2)
ALL_FLAGS = tuple((px, sp, ne) for px in (0, 1) for sp in (0, 1) for ne in (0, 1))
ONE_PASS = 1024 * 256                          # work items of one pass of the grid: sumflux, stage, bdy, halo (see above)
ONE_PASS_MOMENTS = 2048 * 256
MID_SHARE = {f: 0.05 for f in FAMILIES}
MID_SHARE["handles"] = 0.1                     # of 40 cases
SWEEP_FAMILIES = ("ensemble", "handles")      # advance_mu_t runs: its stencil reads one cell past the window
BOX_FAMILIES = ("moments", "diag")            # a box inside memory extents, no domain
VARIANT_COLUMN, VARIANT_MARCH = 1, 2


def per(dtype) -> int:
    """Elements of a 16-byte chunk."""
    return 16 // np.dtype(dtype).itemsize


def bounds_class():
    """synth.Bounds of the package (a dataclass: importing it loads no library)."""
    import __graft_entry__ as g
    return g.load_package().synth.Bounds


@dataclass
class Case:
    family: str
    number: int
    seed: int                                  # of the campaign
    bounds: object
    flags: tuple                               # (periodic_x, specified, nested)
    dtype: type
    members: int
    mid: bool
    params: dict = field(default_factory=dict)

    @property
    def data_seed(self) -> int:
        return (self.seed % 1000003) * 1000 + FAMILIES.index(self.family) * 100000007 + self.number

    def what(self) -> str:
        return (f"seed {self.seed}, family {self.family}, case {self.number}: bounds={self.bounds.as_tuple()} flags={self.flags} "
                f"dtype={np.dtype(self.dtype).name} members={self.members} params={self.params}")


# ---------------------------------------------------------------------------------------------
# the draw
# ---------------------------------------------------------------------------------------------
def _one_of_or_uniform(rng, values, lo, hi):
    return int(rng.choice(values)) if rng.random() < 0.5 else int(rng.integers(lo, hi + 1))


def _sub_range(rng, lo, hi):
    """A sub-range of lo..hi: anchored low, anchored high, one wide, or anywhere."""
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return lo, int(rng.integers(lo, hi + 1))
    if kind == 1:
        return int(rng.integers(lo, hi + 1)), hi
    if kind == 2:
        s = int(rng.integers(lo, hi + 1))
        return s, s
    s = int(rng.integers(lo, hi + 1))
    return s, int(rng.integers(s, hi + 1))


def _mid_dims(rng, family, dtype, axes):
    """(ni, nk, nj) of a mid-sized draw: past one pass of the family's grid with a margin for a trimmed tile."""
    p = per(dtype)
    if family in ("sumflux", "stage"):
        ni, nk = int(rng.integers(9, 41)), int(rng.integers(12, 33))
        chunks = max((ni - 2) // p, 1)                             # of a run shortened by a trimmed tile: a lower bound
        return ni, nk, ONE_PASS // ((nk - 1) * chunks) + 12
    if family == "spec_bdy" or (family == "cyclic" and axes == CR.CYCLIC_X):
        ni, nk = int(rng.integers(2, 7)), int(rng.integers(30, 61))  # one element per run: the column strips and columns
        return ni, nk, ONE_PASS // (nk - 1) + 24
    if family == "cyclic":                                         # rows: levels * chunks of a row
        nk = int(rng.integers(40, 65))
        return p * (ONE_PASS // nk + 8), nk, 1
    if family == "moments":
        ni, nk = int(rng.integers(40, 81)), int(rng.integers(20, 31))
        return ni, nk, ONE_PASS_MOMENTS // (nk * ((ni - 4) // p)) + 12
    if family == "diag":
        return 256 * p + int(rng.integers(1, 71)), int(rng.integers(2, 6)), int(rng.integers(2, 7))
    if family == "handles":                                        # the stage and sumflux launches of the handle go round their grid
        ni, nk = int(rng.integers(257, 331)), int(rng.integers(5, 9))
        return ni, nk, ONE_PASS // (nk * ((ni - 2) // p)) + 12
    return int(rng.integers(257, 331)), int(rng.integers(3, 9)), int(rng.integers(20, 45))


def _flag_sets(family, axes):
    if family == "spec_bdy":
        return tuple(f for f in ALL_FLAGS if f[1] or f[2])
    if family == "cyclic":
        if axes & CR.CYCLIC_Y:
            return tuple(f for f in ALL_FLAGS if not (f[1] or f[2]))
        return tuple(f for f in ALL_FLAGS if f[0] or not (f[1] or f[2]))
    if family in ("sumflux", "stage") or family in BOX_FAMILIES:
        return ((0, 0, 0),)                                        # these calls take no flags
    return ALL_FLAGS


def admitted_flag_sets(family):
    """Every flag set some draw of the family may have."""
    if family == "cyclic":
        return tuple(sorted(set(_flag_sets(family, CR.CYCLIC_X)) | set(_flag_sets(family, CR.CYCLIC_Y))))
    if family == "handles":
        return ALL_FLAGS
    return _flag_sets(family, 0)


# a draw whose contract range is empty is wanted, but rarely: kept this often (the zone update's tiles mostly touch an edge of
# the domain and are seldom empty to begin with)
EMPTY_KEPT = {f: 0.08 for f in FAMILIES}
EMPTY_KEPT["spec_bdy"] = 0.5


def draw(rng, family, number=0, seed=SEED) -> Case:
    """One case of ``family`` from ``rng``.  Draws whose contract range is empty (``empty_contract``) are mostly drawn again,
    from the same generator: they stay under a tenth of a campaign."""
    mid = bool(rng.random() < MID_SHARE[family])
    while True:
        case = _draw_once(rng, family, number, seed, mid)
        if not empty_contract(case) or rng.random() < EMPTY_KEPT[family]:
            return case


def _draw_once(rng, family, number, seed, mid) -> Case:
    assert family in FAMILIES, family
    B = bounds_class()
    dtype = F64 if rng.random() < 0.5 else F32
    sweep, box = family in SWEEP_FAMILIES, family in BOX_FAMILIES
    axes = int(rng.integers(1, 4)) if family == "cyclic" else 0
    ni = _one_of_or_uniform(rng, NI_SET, 1, 70)
    nk = _one_of_or_uniform(rng, NK_SET, 1, 9)
    if nk == 1 and rng.random() < 0.6:                             # one level: t's range is empty; wanted, but rarely
        nk = int(rng.integers(2, 10))
    nj = int(rng.integers(1, 7))
    members = int(rng.integers(2, 5)) if family == "ensemble" else int(rng.integers(1, 5))
    if mid:
        ni, nk, nj = _mid_dims(rng, family, dtype, axes)
        members = 2 if family in ("ensemble", "moments") else 1
    ids, jds = 1, 1
    ide, jde = ids + ni, jds + nj                                  # ni x nj mass points, one more staggered
    kde = nk + 1 if sweep else nk                                  # the streaming calls: nk w levels, nk - 1 of t
    need_i = sweep or bool(axes & CR.CYCLIC_X)                     # memory has to hold column ids - 1 / row jds - 1
    need_j = sweep or bool(axes & CR.CYCLIC_Y)
    ims = ids - int(rng.integers(1 if need_i else 0, 10))
    ime = ide + int(rng.integers(0, 10))
    jms = jds - int(rng.integers(1 if need_j else 0, 4))
    jme = jde + int(rng.integers(0, 4))
    kms = int(rng.choice(KMS_SET))
    kme = kde + int(rng.integers(0, 3))
    if mid:                                                        # keep a mid-sized array small: little padding
        ims, ime, jms, jme = max(ims, ids - 2), min(ime, ide + 1), max(jms, jds - 1), min(jme, jde + 1)
    flag_sets = _flag_sets(family, axes)
    flags = flag_sets[int(rng.integers(0, len(flag_sets)))]
    params = {}
    # the tile: the whole domain half of the time, otherwise a sub-tile as an OpenMP tile or a patch would be
    its, ite, jts, jte = ids, ide, jds, jde
    if box:
        rank = 3 if rng.random() < 0.7 else 2
        whole = rng.random() < 0.2
        its, ite = (ims, ime) if whole else _sub_range(rng, ims, ime)
        jts, jte = (jms, jme) if whole else _sub_range(rng, jms, jme)
        k0, k1 = (kms, kme) if whole else _sub_range(rng, kms, kme)
        if mid:                                                    # the box is most of the array
            its, ite, jts, jte, k0, k1 = ims + int(rng.integers(0, 3)), ime - int(rng.integers(0, 3)), jms, jme, kms, kme
        params.update(rank=rank, k0=k0, k1=k1)
    elif mid:
        if rng.random() < 0.5 and family != "cyclic":
            its, ite = ids + int(rng.integers(0, 2)), ide - int(rng.integers(0, 2))
            jts, jte = jds + int(rng.integers(0, 2)), jde - int(rng.integers(0, 2))
    elif rng.random() < 0.5:
        sub_i, sub_j = rng.random() < 0.6, rng.random() < 0.6
        if family == "cyclic":                                     # a wrapped direction is held whole by the patch
            sub_i, sub_j = sub_i and not (axes & CR.CYCLIC_X), sub_j and not (axes & CR.CYCLIC_Y)
            if axes & CR.CYCLIC_X and rng.random() < 0.5:
                ite = ide - 1                                      # the window decides, not ite
            if axes & CR.CYCLIC_Y and rng.random() < 0.5:
                jte = jde - 1
        if sub_i:
            its, ite = _sub_range(rng, ids, ide)
        if sub_j:
            jts, jte = _sub_range(rng, jds, jde)
        if family == "spec_bdy" and rng.random() < 0.6:            # most tiles of interest touch an edge of the domain
            edge = int(rng.integers(0, 4))
            its, ite, jts, jte = (ids if edge == 0 else its, ide if edge == 1 else ite, jds if edge == 2 else jts,
                                  jde if edge == 3 else jte)
    b = B(ids, ide, jds, jde, kde, ims, ime, jms, jme, kms, kme, its, ite, jts, jte, 1, kde)
    # the family's own parameters
    if family == "ensemble":
        params.update(register=bool(number % 5 == 4))
    elif family == "cyclic":
        params.update(axes=axes)
    elif family == "spec_bdy":
        params.update(dts=float(rng.uniform(0.2, 20.0)))
    elif family == "sumflux":
        params.update(n=1 if mid else int(rng.integers(1, 5)))
    elif family == "stage":
        params.update(rk_step=int(rng.integers(1, 4)), n=int(rng.integers(1, 5)), with_h=bool(rng.integers(0, 2)),
                      dts=float(rng.uniform(0.2, 20.0)))
    elif family == "moments":
        want = [k for k in MR.NAMES if rng.random() < 0.5] or [MR.NAMES[int(rng.integers(0, 4))]]
        params.update(want=tuple(want))
    elif family == "diag":
        params.update(planted=int(rng.integers(0, 7)))
    elif family == "handles":
        px, sp, ne = flags
        clipped = bool(sp or ne)
        whole_i = its == ids and ite >= ide - 1
        whole_j = jts == jds and jte >= jde - 1
        ax = 0
        if whole_i and (px or not clipped) and rng.random() < 0.6:
            ax |= CR.CYCLIC_X
        if whole_j and not clipped and rng.random() < 0.6:
            ax |= CR.CYCLIC_Y
        params.update(kind="ensemble" if rng.random() < 0.5 and not mid else "domain", axes=ax, spec_bdy=bool(clipped and rng.random() < 0.7),
                      sumflux=int(rng.integers(0, 4)), stage=bool(rng.random() < 0.7), sweeps=int(rng.integers(1, 4)),
                      rk_step=int(rng.integers(1, 4)), with_h=bool(rng.integers(0, 2)))
        members = 1 if params["kind"] == "domain" else int(rng.integers(2, 5))
        if mid:
            params.update(sweeps=1, stage=True, sumflux=max(params["sumflux"], 1))
    return Case(family, number, seed, b, flags, dtype, members, mid, params)


def cases(family, count=None, seed=None):
    """The campaign of a family: ``count`` cases of one generator seeded with (seed, family)."""
    seed = SEED if seed is None else seed
    count = N_CASES[family] if count is None else count
    rng = np.random.default_rng([seed, FAMILIES.index(family)])
    for number in range(count):
        yield draw(rng, family, number, seed)


# ---------------------------------------------------------------------------------------------
# what a case is: the properties the coverage test counts
# ---------------------------------------------------------------------------------------------
def run_geometry(case):
    """(elements between the row's first memory column and the run's first element, elements of the run): the contiguous run
    the family's kernels cut into 16-byte chunks."""
    b = case.bounds
    if case.family in BOX_FAMILIES or case.family == "sumflux":
        return b.its - b.ims, b.ite - b.its + 1
    return b.its - b.ims, min(b.ite, b.ide - 1) - b.its + 1


def member_stride_off_16(case) -> bool:
    b = case.bounds
    return case.members > 1 and ((b.idim * b.kdim * b.jdim) % per(case.dtype) != 0 or (b.idim * b.jdim) % per(case.dtype) != 0)


def bdy_strips(b, flags):
    """The strips amt_bdy.hip cuts the zone into, (i0, i1, j0, j1) each."""
    w = SB.window(flags, b)
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    if ihi < b.its or jhi < b.jts:
        return []
    if w[1] < w[0] or w[3] < w[2]:
        return [(b.its, ihi, b.jts, jhi)]
    out = []
    if w[2] > b.jts:
        out.append((b.its, ihi, b.jts, w[2] - 1))
    if w[3] < jhi:
        out.append((b.its, ihi, w[3] + 1, jhi))
    if w[0] > b.its:
        out.append((b.its, w[0] - 1, w[2], w[3]))
    if w[1] < ihi:
        out.append((w[1] + 1, ihi, w[2], w[3]))
    return out


def work_items(case, family=None) -> int:
    """Work items of the job that decides whether the family's launch goes round its grid more than once (the SMALLEST 3-D job
    where a launch has several of one shape, so that every one of them iterates)."""
    b, p, family = case.bounds, per(case.dtype), family or case.family
    chunks = lambda n: -(-max(n, 0) // p)
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    if family == "sumflux":
        return (b.kte - b.kts + 1) * max(b.jte - b.jts + 1, 0) * chunks(b.ite - b.its + 1)
    if family == "stage":
        return (b.kte - b.kts) * max(jhi - b.jts + 1, 0) * chunks(ihi - b.its + 1)
    if case.family == "spec_bdy":
        return max([(j1 - j0 + 1) * (b.kte - b.kts) * chunks(i1 - i0 + 1) for i0, i1, j0, j1 in bdy_strips(b, case.flags)] or [0])
    if case.family == "cyclic":
        i0, i1, j0, j1 = CR.window(case.flags, b)
        if i1 < i0 or j1 < j0:
            return 0
        ax = case.params["axes"]
        return max((j1 - j0 + 1) * b.kdim if ax & CR.CYCLIC_X else 0, b.kdim * chunks(i1 - i0 + 1) if ax & CR.CYCLIC_Y else 0)
    if case.family == "moments":
        nk = case.params["k1"] - case.params["k0"] + 1 if case.params["rank"] == 3 else 1
        return nk * (b.jte - b.jts + 1) * chunks(b.ite - b.its + 1)
    raise ValueError(case.family)


def grid_stride(case) -> bool:
    """Does a launch of this case go round its grid more than once (see the module's docstring)?"""
    b, p = case.bounds, per(case.dtype)
    if case.family == "handles":                                   # the handle's stage and sumflux launches; see the docstring
        return (b.ide - b.ids >= 257 and case.params["stage"] and case.params["sumflux"] > 0
                and min(work_items(case, "stage"), work_items(case, "sumflux")) > ONE_PASS)
    if case.family == "ensemble":
        return b.ide - b.ids >= 257 and b.jde - b.jds >= 2
    if case.family == "diag":
        nchunk = -(-(b.ite - b.its + 1) // p)
        shift = 0
        while shift < 8 and (1 << shift) < nchunk:
            shift += 1
        runs = (case.params["k1"] - case.params["k0"] + 1 if case.params["rank"] == 3 else 1) * (b.jte - b.jts + 1)
        groups = -(-runs // (256 >> shift))
        return groups > min(max(-(-groups // 4), 1), 2048) and nchunk > 256
    return work_items(case) > (ONE_PASS_MOMENTS if case.family == "moments" else ONE_PASS)


def empty_contract(case) -> bool:
    """Nothing may be written: no mass column in the tile, an empty zone, an empty window, or (stage) one level, where t's
    range kts..kte-1 is empty."""
    b = case.bounds
    ihi, jhi = min(b.ite, b.ide - 1), min(b.jte, b.jde - 1)
    if case.family in BOX_FAMILIES:
        return False
    if case.family == "sumflux":
        return False                                               # the tile box always holds a cell, and iteration 1 writes it
    if ihi < b.its or jhi < b.jts:
        return True
    if case.family == "stage":
        return b.kte - b.kts < 1
    if case.family == "spec_bdy":
        return not SB.zone_mask(case.flags, b).any()
    i0, i1, j0, j1 = CR.window(case.flags, b)
    return i1 < i0 or j1 < j0


# ---------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------
def nan_patterns(shape, dtype, tag):
    """Quiet NaNs, every cell with a payload of its own (modulo the payload bits of the type)."""
    wide = np.dtype(dtype).itemsize == 8
    u = np.uint64 if wide else np.uint32
    quiet = u(0x7FF8000000000000) if wide else u(0x7FC00000)
    n = int(np.prod(shape))
    payload = (np.arange(n, dtype=np.uint64) + np.uint64(4099 * tag)) % np.uint64((1 << 22) - 1) + np.uint64(1)
    return (quiet | payload.astype(u)).reshape(shape).view(dtype)


def _stack(shape, members):
    return ((members,) + tuple(shape)) if members > 1 else tuple(shape)


def _fill(a, mask, rng, lo, hi):
    mask = np.broadcast_to(mask, a.shape)
    a[mask] = rng.uniform(lo, hi, int(mask.sum())).astype(a.dtype)
    return a


def shape3(b):
    return (b.jdim, b.kdim, b.idim)


def shape2(b):
    return (b.jdim, b.idim)


def sumflux_read_mask(b, name):
    acc = {"u": "ru_m", "u_1": "ru_m", "muu": "ru_m", "msfuy": "ru_m", "v": "rv_m", "v_1": "rv_m", "muv": "rv_m",
           "msfvx_inv": "rv_m", "ww": "ww_m", "ww_1": "ww_m"}[name]
    m = SF.range_mask(b, acc)
    return m.any(axis=1) if name in SF.INPUTS[6:] else m


def sumflux_inputs(case, iteration):
    b, rng = case.bounds, np.random.default_rng([case.data_seed, iteration])
    out = {}
    for k, name in enumerate(SF.INPUTS):
        two = name in SF.INPUTS[6:]
        a = nan_patterns(_stack(shape2(b) if two else shape3(b), case.members), case.dtype, 3 + k).copy()
        out[name] = _fill(a, sumflux_read_mask(b, name), rng, *((0.5, 1.5) if two else (-2.0, 2.0)))
    return out


def sumflux_poison(case):
    return {n: nan_patterns(_stack(shape3(case.bounds), case.members), case.dtype, k).copy() for k, n in enumerate(SF.ACCUMULATORS)}


STAGE_ALL13 = ST.PREP + ("h_diabatic",)


def stage_read_mask(b, name, rk_step):
    t, ww, col = ST.cell_mask(b, "t"), ST.cell_mask(b, "ww"), ST.column_mask(b)
    masks = {"t": t, "ww": ww, "mu": col, "mut": col, "mub": col, "h_diabatic": t}
    if rk_step > 1:
        masks.update(t_old=t, mu_old=col)
    return masks.get(name)


def stage_state(case):
    """As _state of tests/test_gpu_39_stage.py: at rk_step 1 t_old, t_1, ww_1, mu_old, mu_save, muts and mudf are all poison."""
    b, rng = case.bounds, np.random.default_rng([case.data_seed, 0])
    out = {}
    for k, name in enumerate(STAGE_ALL13):
        two = name in ST.PREP_2D
        a = nan_patterns(_stack(shape2(b) if two else shape3(b), case.members), case.dtype, k).copy()
        mask = stage_read_mask(b, name, case.params["rk_step"])
        out[name] = a if mask is None else _fill(a, mask, rng, *((0.5, 1.5) if two else (-2.0, 2.0)))
    return out


BDY_NAMES = ("t", "ft", "mu", "muts", "mu_tend")


def bdy_state(case):
    b, rng = case.bounds, np.random.default_rng([case.data_seed, 0])
    zone = SB.zone_mask(case.flags, b)
    zone3 = np.zeros(shape3(b), bool)
    zone3[:, b.kts - b.kms:b.kte - b.kms, :] = zone[:, None, :]
    out = {}
    for k, name in enumerate(BDY_NAMES):
        two = name in ("mu", "muts", "mu_tend")
        a = nan_patterns(_stack(shape2(b) if two else shape3(b), case.members), case.dtype, k).copy()
        out[name] = _fill(a, zone if two else zone3, rng, -2.0, 2.0)
    return out


def cyclic_state(case):
    """A copy moves bits: every cell a NaN payload of its own, and random finite values in about half of them (payloads alone
    in a mid-sized draw)."""
    b, rng = case.bounds, np.random.default_rng([case.data_seed, 0])
    out = {}
    for k, name in enumerate(CR.MAY_CHANGE):
        a = nan_patterns(_stack(shape3(b) if name in CR.RANK3 else shape2(b), case.members), case.dtype, k).copy()
        out[name] = a if case.mid else _fill(a, rng.random(a.shape) < 0.5, rng, -2.0, 2.0)
    return out


def box_extents(case):
    b = case.bounds
    return (b.ims, b.ime, b.jms, b.jme, b.kms, b.kme)


def box_of(case):
    b = case.bounds
    return (b.its, b.ite, case.params["k0"], case.params["k1"], b.jts, b.jte)


def _box_shape(case):
    b = case.bounds
    return shape3(b) if case.params["rank"] == 3 else shape2(b)


def moments_state(case):
    """The stacked input: random inside the box (a member's own scale, so that the spread is not small), poison outside; and
    the four outputs, poison everywhere."""
    rng = np.random.default_rng([case.data_seed, 0])
    one = _box_shape(case)
    a = nan_patterns((case.members,) + one, case.dtype, 0).copy()
    idx = DR.box_index(a[0], box_extents(case), box_of(case))
    for m in range(case.members):
        a[m][idx] = (rng.standard_normal(a[m][idx].shape) * 10.0 ** rng.uniform(-2, 3) + rng.uniform(-50, 50)).astype(case.dtype)
    outs = {name: nan_patterns(one, case.dtype, 1 + k).copy() for k, name in enumerate(MR.NAMES) if name in case.params["want"]}
    return a, outs


def diag_state(case):
    """Two stacked arrays: random values, ``b`` a copy of ``a``; then NaN, Inf and single-bit flips planted at random
    positions of the whole arrays, inside the box and outside."""
    rng = np.random.default_rng([case.data_seed, 0])
    shape = (case.members,) + _box_shape(case)
    a = (rng.standard_normal(shape) * 300.0 + 250.0).astype(case.dtype)
    bb = a.copy()
    u = np.uint64 if np.dtype(case.dtype).itemsize == 8 else np.uint32
    bits = 8 * np.dtype(case.dtype).itemsize
    fa, fb = a.reshape(-1), bb.reshape(-1)
    for _ in range(case.params["planted"]):
        at, kind = int(rng.integers(0, fa.size)), int(rng.integers(0, 4))
        if kind == 0:
            fa[at] = np.nan
        elif kind == 1:
            fa[at] = np.inf if rng.random() < 0.5 else -np.inf
            fb[at] = fa[at] if rng.random() < 0.5 else fb[at]
        elif kind == 2:
            fb.view(u)[at] ^= u(1) << u(int(rng.integers(0, bits)))
        else:
            fa.view(u)[at] = u(0x7FF0000000ABCDEF) if bits == 64 else u(0x7F80BEEF)      # a NaN with a payload
    return a, bb


# ---------------------------------------------------------------------------------------------
# the vectorised twin of sumflux_ref.sumflux (explicit loops there: too slow for a mid-sized draw).  The CPU test holds the
# two bit-equal on every small draw of the campaign.
# ---------------------------------------------------------------------------------------------
def sumflux_vec(acc, inp, b, first, last, n, members=1):
    with np.errstate(all="ignore"):
        for name in SF.ACCUMULATORS:
            xn, x1n, fan, fbn = SF.ROLE[name]
            a = acc[name]
            T = a.dtype.type
            tile = np.broadcast_to(SF.tile_mask(b), a.shape)
            rng_ = np.broadcast_to(SF.range_mask(b, name), a.shape)
            if first:
                a[tile & ~rng_] = T(0)
            i0, i1, k0, k1, j0, j1 = SF.ranges(b, name)
            if i1 < i0 or k1 < k0 or j1 < j0:
                continue
            box = (Ellipsis, slice(j0 - b.jms, j1 - b.jms + 1), slice(k0 - b.kms, k1 - b.kms + 1), slice(i0 - b.ims, i1 - b.ims + 1))
            flat = (Ellipsis, box[1], None, box[3])
            x = inp[xn][box]
            s = (T(0) + x) if first else (a[box] + x)
            if last:
                q = s / T(n)
                x1 = inp[x1n][box]
                if name == "ru_m":
                    s = q + (inp[fan][flat] * x1) / inp[fbn][flat]
                elif name == "rv_m":
                    s = q + (inp[fan][flat] * x1) * inp[fbn][flat]
                else:
                    s = q + x1
            a[box] = s
    return acc


# ---------------------------------------------------------------------------------------------
# the references as ops
# ---------------------------------------------------------------------------------------------
class RefOps:
    """The numpy references of the tree (and the C oracle for a sweep), one method per library call, IN PLACE."""

    def __init__(self, pkg=None, oracle=None):
        self.pkg, self.oracle = pkg, oracle

    # a: the ensemble launch.  Every member alone through the oracle.  Returns the status (0)
    def sweep(self, stacked, case, variant, scalars):
        S = self.pkg.synth
        cfg = self.pkg.GridConfig(*[bool(x) for x in case.flags])
        for m in range(case.members):
            one = {n: (a if S.field_rank(n) == 1 else a[m]) for n, a in stacked.items()}
            self.oracle.advance_mu_t(*S.Patch(case.bounds, cfg, one, *scalars).args())
        return 0

    def cyclic(self, arrays, case):
        CR.cyclic_fill(arrays, case.bounds, case.params["axes"], case.flags)

    def spec_bdy(self, arrays, case):
        SB.spec_bdy_update(arrays, case.bounds, case.flags, case.params["dts"])

    def sumflux(self, acc, inp, case, iteration, n):
        if case.mid:
            sumflux_vec(acc, inp, case.bounds, iteration == 1, iteration == n, n, case.members)
        else:
            SF.sumflux(acc, inp, case.bounds, iteration, n, case.members)

    def prep(self, a, case, rk_step):
        ST.prep(a, case.bounds, rk_step)

    def finish(self, a, case, n, dts, with_h):
        ST.finish(a, case.bounds, n, dts, a["h_diabatic"] if with_h else None)

    def moments(self, a, outs, case):
        ext, box = box_extents(case), box_of(case)
        ref = MR.moments(a, ext, box)
        idx = MR.member_index(a, ext, box)
        for name in outs:
            outs[name][...] = MR.expected(outs[name], ref[name], idx)

    def stats(self, a, case):
        return [DR.stats(a[m], box_extents(case), box_of(case)) for m in range(case.members)]

    def compare(self, a, bb, case):
        return [DR.diff(a[m], bb[m], box_extents(case), box_of(case)) for m in range(case.members)]

    def stage_on_handle(self, case, fields, extras, acc, scalars):
        """prep -> (new inputs, cyclic refresh, oracle sweep, zone update, accumulation) x sweeps -> finish, on the host."""
        p, S = case.params, self.pkg.synth
        cfg = self.pkg.GridConfig(*[bool(x) for x in case.flags])
        everything = dict(fields, **extras)
        n = p["sweeps"]
        if p["stage"]:
            ST.prep(everything, case.bounds, p["rk_step"])
        for s in range(n):
            refresh_exchanged(case, self.pkg, fields, scalars, s)
            if p["axes"]:
                CR.cyclic_fill(fields, case.bounds, p["axes"], case.flags)
            for m in range(case.members):
                one = {k: (a if S.field_rank(k) == 1 or case.members == 1 else a[m]) for k, a in fields.items()}
                self.oracle.advance_mu_t(*S.Patch(case.bounds, cfg, one, *scalars).args())
            if p["spec_bdy"]:
                SB.spec_bdy_update(fields, case.bounds, case.flags, scalars[2])
            if p["sumflux"]:
                self.sumflux(acc, fields, case, s % p["sumflux"] + 1, p["sumflux"])
        if p["stage"]:
            ST.finish(everything, case.bounds, n, scalars[2], extras["h_diabatic"] if p["with_h"] else None)


# ---------------------------------------------------------------------------------------------
# the scripts
# ---------------------------------------------------------------------------------------------
def _snap(arrays):
    return {n: (a.copy() if isinstance(a, np.ndarray) else a) for n, a in arrays.items() if a is not None}


def sweep_read_masks(case, pkg, one):
    """name -> bool array over ONE patch's arrays: the cells advance_mu_t reads as inputs (tests/special_values.py)."""
    import special_values as SV
    return SV.read_mask(pkg.synth.Patch(case.bounds, pkg.GridConfig(*[bool(x) for x in case.flags]), one))


def handles_read_masks(case, pkg, one):
    """The cells ANY call of the case's composition reads before the composition has written them, a union over the sweep,
    the cyclic refresh, the zone update, the accumulation and the stage bracket (whatever the order of the calls)."""
    b, p, m = case.bounds, case.params, sweep_read_masks(case, pkg, one)
    i0, i1, j0, j1 = CR.window(case.flags, b)
    if p["axes"] and i1 >= i0 and j1 >= j0:                        # the cells a refresh copies FROM
        J, I = slice(j0 - b.jms, j1 - b.jms + 1), slice(i0 - b.ims, i1 - b.ims + 1)
        if p["axes"] & CR.CYCLIC_X:
            for n in CR.COLS_FROM_RIGHT:
                m[n][J, ..., b.ids - b.ims] = True
            m["t_1"][J, :, b.ide - 1 - b.ims] = True
        if p["axes"] & CR.CYCLIC_Y:
            for n in CR.ROWS_FROM_ABOVE:
                m[n][b.jds - b.jms, ..., I] = True
            m["t_1"][b.jde - 1 - b.jms, :, I] = True
    if p["spec_bdy"]:
        zone = SB.zone_mask(case.flags, b)
        for n in ("mu", "muts", "mu_tend"):
            m[n] |= zone
        for n in ("t", "ft"):
            m[n][:, b.kts - b.kms:b.kte - b.kms, :] |= zone[:, None, :]
    if p["sumflux"]:
        for n in SF.INPUTS:
            m[n] |= sumflux_read_mask(b, n)
    if p["stage"]:
        m["t"] |= ST.cell_mask(b, "t")
        m["ww"] |= ST.cell_mask(b, "ww")
        for n in ("mu", "mut"):
            m[n] |= ST.column_mask(b)
    return m


def poison_unread(one, masks, member, names=None):
    """NaN with a payload of its own into every cell of ONE patch's arrays that ``masks`` leaves out."""
    for k, n in enumerate(sorted(masks)):
        if names is None or n in names:
            keep = masks[n]
            one[n][~keep] = nan_patterns(one[n].shape, one[n].dtype, 40 * member + k)[~keep]


def ensemble_state(case, pkg, read_masks=sweep_read_masks):
    """The 26 member-stacked arrays (the 1-D ones shared) and the four scalars: member m is make_patch with seed + m, then
    poisoned in every cell the calls of the case do not read."""
    S, b = pkg.synth, case.bounds
    dims = (b.ide - b.ids, b.kde - 1, b.jde - b.jds)
    cfg = pkg.GridConfig(*[bool(x) for x in case.flags])
    patches = [S.make_patch(b, cfg, dtype=case.dtype, seed=case.data_seed % (1 << 31) + m, global_dims=dims) for m in range(case.members)]
    for m, q in enumerate(patches):
        poison_unread(q.arrays, read_masks(case, pkg, q.arrays), m)
    stacked = {n: (patches[0].arrays[n].copy() if S.field_rank(n) == 1 else np.stack([q.arrays[n] for q in patches])) for n in S.FIELD_NAMES}
    p = patches[0]
    return stacked, (p.rdx, p.rdy, p.dts, p.epssm, dims)


def run(case, ops, pkg=None):
    """Play the family's script through ``ops``: [(label, {name: whole array or list of records})], one entry per call.  An
    entry is (label, None) where ops declined the call (no march shape for a level count)."""
    f, out = case.family, []
    if f == "ensemble":
        start, scalars = ensemble_state(case, pkg)
        for variant, label in ((VARIANT_MARCH, "march"), (VARIANT_COLUMN, "column")):
            arrays = {n: a.copy() for n, a in start.items()}
            status = ops.sweep(arrays, case, variant, scalars)
            out.append((label, _snap(arrays) if status == 0 else None))
    elif f == "cyclic":
        arrays = cyclic_state(case)
        ops.cyclic(arrays, case)
        out.append(("cyclic_fill", _snap(arrays)))
    elif f == "spec_bdy":
        arrays = bdy_state(case)
        ops.spec_bdy(arrays, case)
        out.append(("spec_bdy_update", _snap(arrays)))
    elif f == "sumflux":
        n, acc = case.params["n"], sumflux_poison(case)
        for it in range(1, n + 1):
            inp = sumflux_inputs(case, it)
            ops.sumflux(acc, inp, case, it, n)
            out.append((f"iteration {it} of {n}", _snap(dict(acc, **inp))))
    elif f == "stage":
        p, a = case.params, stage_state(case)
        ops.prep(a, case, p["rk_step"])
        out.append((f"prep {p['rk_step']}", _snap(a)))
        ops.finish(a, case, p["n"], p["dts"], p["with_h"])
        out.append((f"finish n={p['n']} h={p['with_h']}", _snap(a)))
    elif f == "moments":
        a, outs = moments_state(case)
        ops.moments(a, outs, case)
        out.append(("moments", _snap(dict(outs, a=a))))
    elif f == "diag":
        a, bb = diag_state(case)
        out.append(("field_stats", dict(records=ops.stats(a, case), a=a.copy())))
        out.append(("compare", dict(records=ops.compare(a, bb, case), a=a.copy(), b=bb.copy())))
    elif f == "handles":
        out = run_handles(case, ops, pkg)
    else:
        raise ValueError(f)
    return out


# ---------------------------------------------------------------------------------------------
# h: composition on the handles.  The device side is ONE op, ``ops.stage_on_handle``; the host side composes the references as
# test_three_stages_of_a_time_step_on_a_domain of tests/test_gpu_39_stage.py does.
# ---------------------------------------------------------------------------------------------
def handles_extras(case, stacked_mu):
    """t_old, mu_old, mu_save poisoned, mub so large that muts stays positive, a diabatic heating (as _extras of test_gpu_39)."""
    b, rng = case.bounds, np.random.default_rng([case.data_seed, 1])
    s3, s2 = _stack(shape3(b), case.members), _stack(shape2(b), case.members)
    out = {name: nan_patterns(s3 if name == "t_old" else s2, case.dtype, 5 + k).copy() for k, name in enumerate(("t_old", "mu_old", "mu_save"))}
    finite = np.abs(stacked_mu[np.isfinite(stacked_mu)])            # (mu is poisoned where nothing reads it)
    out["mub"] = (2.0 * (finite.max() if finite.size else 0.0) + 1.0 + rng.uniform(0.0, 1.0, s2)).astype(case.dtype)
    out["h_diabatic"] = rng.uniform(-1e-3, 1e-3, s3).astype(case.dtype)
    return out


def handles_state(case, pkg):
    """(fields, extras, accumulators, scalars): member-stacked where members > 1, one patch's shapes for a domain."""
    stacked, scalars = ensemble_state(case, pkg, handles_read_masks)
    if case.members == 1:
        stacked = {n: (a if pkg.synth.field_rank(n) == 1 else a[0]) for n, a in stacked.items()}
    extras = handles_extras(case, stacked["mu"])
    if case.params["rk_step"] > 1:                                 # a later stage: t_old, mu_old hold the step's start
        rng = np.random.default_rng([case.data_seed, 2])
        extras["t_old"] = rng.uniform(-2.0, 2.0, extras["t_old"].shape).astype(case.dtype)
        extras["mu_old"] = rng.uniform(-0.5, 0.5, extras["mu_old"].shape).astype(case.dtype)
    acc = sumflux_poison(case)
    return stacked, extras, acc, scalars


def refresh_exchanged(case, pkg, fields, scalars, sweep):
    """New exchanged inputs of sweep ``sweep`` in every member -- poisoned again where nothing reads them --, t_1 left alone
    (it is prep's)."""
    S, b = pkg.synth, case.bounds
    cfg = pkg.GridConfig(*[bool(x) for x in case.flags])
    for m in range(case.members):
        one = {n: (a if S.field_rank(n) == 1 or case.members == 1 else a[m]) for n, a in fields.items()}
        keep = one["t_1"].copy()
        S.refresh_exchanged_inputs(S.Patch(b, cfg, one, *scalars), case.data_seed % (1 << 31) + m, sweep + 1)
        one["t_1"][...] = keep
        poison_unread(one, handles_read_masks(case, pkg, one), m, [n for n in S.EXCHANGED_INPUTS if n != "t_1"])


def run_handles(case, ops, pkg):
    fields, extras, acc, scalars = handles_state(case, pkg)
    ops.stage_on_handle(case, fields, extras, acc, scalars)
    return [("stage on a handle", _snap(dict(fields, **{f"extra:{k}": v for k, v in extras.items()},
                                              **{f"acc:{k}": v for k, v in acc.items()})))]


# ---------------------------------------------------------------------------------------------
# the comparison
# ---------------------------------------------------------------------------------------------
def bits_equal(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _record_difference(got, want):
    """Two records of diag_ref's keys: counts, offsets, min, max, max-abs equal; the sum within diag_ref.sum_bound."""
    for k, w in want.items():
        if k == "abs_sum":
            continue
        g = got[k]
        if k == "sum":
            bound = DR.sum_bound(want["count"], want["abs_sum"])
            if not abs(g - w) <= bound:
                return f"sum {g!r} vs fsum {w!r}: off by {abs(g - w):.3e} > {bound:.3e}"
        elif g != w:
            return f"{k} = {g!r}, the reference has {w!r}"
    return None


def first_difference(case, got, want):
    """None where the two plays of a script agree -- every array whole and as bytes, every record as diag_ref compares it --,
    else the text of the first difference, with the case's seed, number and bounds.  A call ``got`` declined is no difference."""
    assert [l for l, _ in got] == [l for l, _ in want], (case.what(), [l for l, _ in got], [l for l, _ in want])
    for (label, g), (_l, w) in zip(got, want):
        if g is None or w is None:
            continue
        assert sorted(g) == sorted(w), (case.what(), label, sorted(g), sorted(w))
        for name in w:
            if name == "records":
                if len(g[name]) != len(w[name]):
                    return f"{case.what()}: {label}: {len(g[name])} records for {len(w[name])} members"
                for m, (gr, wr) in enumerate(zip(g[name], w[name])):
                    d = _record_difference(gr, wr)
                    if d:
                        return f"{case.what()}: {label}, member {m}: {d}"
            elif not bits_equal(g[name], w[name]):
                bad = np.argwhere(_as_uint(g[name]) != _as_uint(w[name]))
                return (f"{case.what()}: {label}: {name} differs from the reference in {len(bad)} cells, first at "
                        f"{tuple(int(x) for x in bad[0])}")
    return None


def _as_uint(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype.itemsize == 8 else np.uint32)


# ---------------------------------------------------------------------------------------------
# mutants: deliberately wrong references, each the shape of a bug these kernels could plausibly have.  Only the CPU test plays
# them; nothing wrong is ever run on a device.
# ---------------------------------------------------------------------------------------------
@contextmanager
def _patched(obj, name, value):
    old = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, old)


def _with_bounds(case, **kw):
    return Case(case.family, case.number, case.seed, case.bounds.replace(**kw), case.flags, case.dtype, case.members, case.mid,
                case.params)


def _member_views(arrays, members, stride_short):
    """Member m of every stacked array as the kernel would see it with a member stride ``stride_short`` elements short."""
    for m in range(members):
        one = {}
        for n, a in arrays.items():
            size = a[0].size
            flat = a.reshape(-1)
            at = m * (size - stride_short)
            one[n] = flat[at:at + size].reshape(a[0].shape)
        yield one


class _Mutant(RefOps):
    family = None
    what = ""


class ClipAtIde(_Mutant):
    family, what = "stage", "clip at ide instead of ide-1"

    def prep(self, a, case, rk_step):
        RefOps.prep(self, a, _with_bounds(case, ide=case.bounds.ide + 1), rk_step)

    def finish(self, a, case, n, dts, with_h):
        RefOps.finish(self, a, _with_bounds(case, ide=case.bounds.ide + 1), n, dts, with_h)


class ClipAtJde(_Mutant):
    family, what = "sumflux", "clip at jde instead of jde-1"

    def sumflux(self, acc, inp, case, iteration, n):
        RefOps.sumflux(self, acc, inp, _with_bounds(case, jde=case.bounds.jde + 1), iteration, n)


class TOverKte(_Mutant):
    family, what = "stage", "t over kts..kte instead of kts..kte-1"

    @staticmethod
    def _boxes(b):
        col, _cell_t, cell_w, lift = TOverKte.real(b)
        return col, cell_w, cell_w, lift

    def prep(self, a, case, rk_step):
        with _patched(ST, "_boxes", self._boxes):
            RefOps.prep(self, a, case, rk_step)

    def finish(self, a, case, n, dts, with_h):
        with _patched(ST, "_boxes", self._boxes):
            RefOps.finish(self, a, case, n, dts, with_h)


TOverKte.real = staticmethod(ST._boxes)


class WwShortOfKte(_Mutant):
    family, what = "stage", "ww over kts..kte-1 instead of kts..kte"

    @staticmethod
    def _boxes(b):
        col, cell_t, _cell_w, lift = TOverKte.real(b)
        return col, cell_t, cell_t, lift

    prep, finish = TOverKte.prep, TOverKte.finish


class LastMemberSkipped(_Mutant):
    family, what = "sumflux", "the last member skipped"

    def sumflux(self, acc, inp, case, iteration, n):
        if case.members == 1:
            return RefOps.sumflux(self, acc, inp, case, iteration, n)
        fewer = Case(case.family, case.number, case.seed, case.bounds, case.flags, case.dtype, case.members - 1, case.mid, case.params)
        sub = lambda d: {k: (v[:-1] if case.members > 2 else v[0]) for k, v in d.items()}
        RefOps.sumflux(self, sub(acc), sub(inp), fewer, iteration, n)


class MemberStrideShort(_Mutant):
    family, what = "stage", "a member read at stride jdim*kdim*idim - 1"

    def prep(self, a, case, rk_step):
        if case.members == 1:
            return RefOps.prep(self, a, case, rk_step)
        for one in _member_views(a, case.members, 1):
            ST.prep(one, case.bounds, rk_step)

    def finish(self, a, case, n, dts, with_h):
        if case.members == 1:
            return RefOps.finish(self, a, case, n, dts, with_h)
        for one in _member_views(a, case.members, 1):
            ST.finish(one, case.bounds, n, dts, one["h_diabatic"] if with_h else None)


class FullChunkAtTheTail(_Mutant):
    family, what = "sumflux", "a full chunk written where the tail is short"

    def sumflux(self, acc, inp, case, iteration, n):
        b, p = case.bounds, per(case.dtype)
        ni = b.ite - b.its + 1
        ite = min(b.ime, b.its + -(-ni // p) * p - 1)
        RefOps.sumflux(self, acc, inp, _with_bounds(case, ite=ite, ide=max(b.ide, ite + 1)), iteration, n)


class PrepReadsStoredMuts(_Mutant):
    family, what = "stage", "prep reading the stored muts instead of mub + mu"

    def prep(self, a, case, rk_step):
        stored = a["muts"].copy()
        RefOps.prep(self, a, case, rk_step)
        _col, cell_t, _w, lift = ST._boxes(case.bounds)
        with np.errstate(all="ignore"):
            a["t"][cell_t] = stored[lift] * a["t_old"][cell_t] - a["mut"][lift] * a["t_1"][cell_t]


class PrepReadsMuAtLaterSteps(_Mutant):
    family, what = "stage", "prep at rk_step >= 2 reading mu instead of mu_old"

    def prep(self, a, case, rk_step):
        if rk_step == 1:
            return RefOps.prep(self, a, case, rk_step)
        RefOps.prep(self, dict(a, mu_old=a["mu"].copy()), case, rk_step)


class FinishRoundsInDouble(_Mutant):
    family, what = "stage", "finish with dts*n rounded in double for fp32"

    def finish(self, a, case, n, dts, with_h):
        RefOps.finish(self, a, case, 1, float(dts) * n, with_h)     # c = T(dts * n): one rounding, from the double product


class SumfluxFinalisesEarly(_Mutant):
    family, what = "sumflux", "sumflux finalising at iteration n-1"

    def sumflux(self, acc, inp, case, iteration, n):
        sumflux_vec(acc, inp, case.bounds, iteration == 1, iteration == n - 1, n, case.members)


class ZoneWithPeriodicWindow(_Mutant):
    family, what = "spec_bdy", "the zone computed with the periodic_x window when it is not periodic"

    def spec_bdy(self, arrays, case):
        SB.spec_bdy_update(arrays, case.bounds, (1,) + tuple(case.flags[1:]), case.params["dts"])


class CyclicPeriodOneShort(_Mutant):
    # a reading of "the cyclic refresh taking ide-1 from ids+1": the wrap one column off, a period of ide - ids - 1
    family, what = "cyclic", "the cyclic refresh taking column ide from ids+1 (a period one short; ids-1 from ide-1 as it should)"

    def cyclic(self, arrays, case):
        RefOps.cyclic(self, arrays, case)
        b = case.bounds
        if case.params["axes"] & CR.CYCLIC_X:
            _i0, _i1, j0, j1 = CR.window(case.flags, b)
            J = slice(j0 - b.jms, j1 - b.jms + 1)
            for n in CR.COLS_FROM_RIGHT:
                a = arrays[n]
                if n in CR.RANK3:
                    a[..., J, :, b.ide - b.ims] = a[..., J, :, b.ids + 1 - b.ims]
                else:
                    a[..., J, b.ide - b.ims] = a[..., J, b.ids + 1 - b.ims]


class VarianceOverMembers(_Mutant):
    family, what = "moments", "the moments variance divided by members"

    def moments(self, a, outs, case):
        RefOps.moments(self, a, outs, case)
        if "var" in outs and case.members > 1:
            idx = MR.member_index(a, box_extents(case), box_of(case))
            x = [a[m][idx].astype(np.float64) for m in range(case.members)]
            mean = x[0]
            for m in range(1, case.members):
                mean = mean + x[m]
            mean = mean / np.float64(case.members)
            q = np.zeros_like(mean)
            for m in range(case.members):
                q = q + (x[m] - mean) * (x[m] - mean)
            outs["var"][idx] = (q / np.float64(case.members)).astype(a.dtype)


class FirstNanFromTheBox(_Mutant):
    family, what = "diag", "the first-NaN offset counted from the box instead of the array"

    def stats(self, a, case):
        out = RefOps.stats(self, a, case)
        idx = DR.box_index(a[0], box_extents(case), box_of(case))
        for m, rec in enumerate(out):
            bad = ~np.isfinite(a[m][idx].ravel())
            rec["first_nonfinite"] = int(np.flatnonzero(bad)[0]) if bad.any() else -1
        return out


MUTANTS = (ClipAtIde, ClipAtJde, TOverKte, WwShortOfKte, LastMemberSkipped, MemberStrideShort, FullChunkAtTheTail,
           PrepReadsStoredMuts, PrepReadsMuAtLaterSteps, FinishRoundsInDouble, SumfluxFinalisesEarly, ZoneWithPeriodicWindow,
           CyclicPeriodOneShort, VarianceOverMembers, FirstNanFromTheBox)
