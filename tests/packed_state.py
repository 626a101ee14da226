"""TEST INFRASTRUCTURE: a patch's 26 arrays packed back to back into ONE pool, as a host that keeps WRF's state on the device
holds them, and a comparer of whole pools.  Plain numpy, no library calls (``views`` also cuts a torch tensor).

Every other GPU test hands the library arrays that are allocations of their own: each base is 256-byte aligned, two arrays of
one shape always share their phase, and a store just outside an array lands in allocator slack.  Here

* every array sits at an element offset of its own and is bracketed by GUARD BANDS of at least ``idim * kdim + 128`` elements
  (one 3-D j row plus the widest tile: no access the kernels make, their deliberate over-reads included, leaves the pool or
  reaches another array);
* on top of that width every array gets 0 .. 16/itemsize - 1 elements, chosen by ``rotation``, so that over the rotations
  every array takes every phase ``base % 16``, the pairs whose two addresses decide one access width (t/ft, mu/mu_tend,
  muts/mu_tend, t_1/t) never share a phase, and some 3-D array lies on a 16-byte boundary that is no 128-byte line;
* the guards hold NaNs whose payload is the pool index, quiet and signalling in turn: a duplicated or shifted chunk cannot
  compare equal, and a result that depends on a guard element is NaN;
* ``diff`` compares WHOLE pools as bytes and names the first differing region: outputs, inputs that must stay as they were,
  unread levels and guards are one assertion.

The phases are those of the pool's first element plus the offset: the pool itself has to start on a 128-byte line
(``aligned_empty`` on the host; a device allocation does).
"""
from __future__ import annotations

import numpy as np

FIELD_NAMES = ("ww", "ww_1", "u", "u_1", "v", "v_1", "mu", "mut", "muave", "muts", "muu", "muv",
               "mudf", "t", "t_1", "t_ave", "ft", "mu_tend", "dnw", "fnm", "fnp", "rdnw",
               "msfuy", "msfvx_inv", "msftx", "msfty")
RANK3 = ("ww", "ww_1", "u", "u_1", "v", "v_1", "t", "t_1", "t_ave", "ft")
RANK1 = ("dnw", "fnm", "fnp", "rdnw")
TILE = 128                                   # the widest march tile, in columns
LINE = 128                                   # bytes
# the pairs whose two addresses pick ONE access width in a kernel: never on one phase
PAIRS = (("t", "ft"), ("mu", "mu_tend"), ("muts", "mu_tend"), ("t_1", "t"))
# phase (in elements, modulo 16/itemsize) at rotation 0 of the arrays of PAIRS; every other array: its position in `names`
_PHASE0 = {"t": 0, "ft": 1, "t_1": 1, "mu": 0, "muts": 0, "mu_tend": 1}


def field_shape(bounds, name, members=1):
    """(jdim, kdim, idim) / (jdim, idim) / (kdim,), member-stacked arrays with one more leading axis (1-D metrics are shared)."""
    if name in RANK1:
        return (bounds.kdim,)
    one = (bounds.jdim, bounds.kdim, bounds.idim) if name in RANK3 else (bounds.jdim, bounds.idim)
    return ((int(members),) + one) if members > 1 else one


class Layout(dict):
    """name -> element offset of the array's first cell.  ``length``: elements of the pool; ``shapes``: name -> shape;
    ``guard``: the least guard width; ``dtype``; ``members``; ``names``: the arrays in pool order."""

    def size(self, name) -> int:
        return int(np.prod(self.shapes[name]))

    def end(self, name) -> int:
        return self[name] + self.size(name)

    def phase_bytes(self, name) -> int:
        return (self[name] * self.dtype.itemsize) % 16


def layout(bounds, dtype, members=1, rotation=0, names=FIELD_NAMES):
    """``names``: field names (shapes from ``bounds`` and ``members``) or a mapping name -> shape (any arrays)."""
    dt = np.dtype(dtype)
    per = 16 // dt.itemsize
    if not 0 <= int(rotation) < per:
        raise ValueError(f"rotation {rotation}: 0 .. {per - 1} for {dt}")
    shapes = dict(names) if isinstance(names, dict) else {n: field_shape(bounds, n, members) for n in names}
    guard = bounds.idim * bounds.kdim + TILE
    lay = Layout()
    lay.shapes, lay.guard, lay.dtype, lay.members, lay.names = shapes, guard, dt, int(members), tuple(shapes)
    at, off_line = 0, False
    for pos, name in enumerate(lay.names):
        phase = (_PHASE0.get(name, pos) + int(rotation)) % per
        base = at + guard
        base += (phase - base) % per                              # 0 .. per - 1 extra elements
        if not off_line and len(shapes[name]) >= 3 and phase == 0:
            if (base * dt.itemsize) % LINE == 0:
                base += per                                       # a 16-byte boundary that is no 128-byte line: 16 bytes more guard
            off_line = True
        lay[name] = base
        at = base + int(np.prod(shapes[name]))
    lay.length = at + guard
    return lay


def _uint(dt):
    return np.uint64 if np.dtype(dt).itemsize == 8 else np.uint32


def aligned_empty(n, dtype):
    """n elements of ``dtype`` whose first lies on a 128-byte line."""
    dt = np.dtype(dtype)
    raw = np.empty(n * dt.itemsize + LINE, np.uint8)
    skip = (-raw.ctypes.data) % LINE
    return raw[skip:skip + n * dt.itemsize].view(dt)


def guard_pattern(length, dtype):
    """The bits a pool of ``length`` elements holds in its guards: element e a NaN with payload e + 1, quiet for even e and
    signalling for odd e."""
    dt = np.dtype(dtype)
    u = _uint(dt)
    e = np.arange(length, dtype=u)
    if dt.itemsize == 8:
        return np.where(e % u(2) == 0, u(0x7FF8000000000000), u(0x7FF0000000000000)) | (e + u(1))
    if length + 1 >= 1 << 22:
        raise ValueError(f"a float32 pool of {length} elements: the payload has 22 bits")
    return np.where(e % u(2) == 0, u(0x7FC00000), u(0x7F800000)) | (e + u(1))


def place(arrays, lay):
    """A pool (numpy, ``lay.dtype``, on a 128-byte line) with ``arrays[name]`` at ``lay[name]`` and the guard pattern everywhere
    else.  The arrays are copied as bits."""
    u = _uint(lay.dtype)
    pool = aligned_empty(lay.length, lay.dtype)
    bits = pool.view(u)
    bits[:] = guard_pattern(lay.length, lay.dtype)
    for name in lay.names:
        a = np.ascontiguousarray(arrays[name])
        if a.dtype != lay.dtype or tuple(a.shape) != tuple(lay.shapes[name]):
            raise ValueError(f"{name}: {a.dtype} {a.shape}, the layout holds {lay.dtype} {lay.shapes[name]}")
        bits[lay[name]:lay.end(name)] = a.reshape(-1).view(u)
    return pool


def clone(pool):
    """A copy of a numpy pool, again on a 128-byte line."""
    out = aligned_empty(pool.size, pool.dtype)
    out.view(_uint(pool.dtype))[:] = pool.view(_uint(pool.dtype))
    return out


def views(pool, lay, bounds=None, members=None):
    """name -> contiguous view of the array inside ``pool`` (a numpy array or a torch tensor of ``lay.length`` elements).
    ``bounds`` / ``members``, when given, must be those of the layout."""
    if int(pool.shape[0]) != lay.length or len(pool.shape) != 1:
        raise ValueError(f"a pool of shape {tuple(pool.shape)}, the layout has {lay.length} elements")
    if members is not None and int(members) != lay.members:
        raise ValueError(f"members = {members}, the layout has {lay.members}")
    out = {}
    for name in lay.names:
        if bounds is not None and name in FIELD_NAMES and tuple(lay.shapes[name]) != field_shape(bounds, name, lay.members):
            raise ValueError(f"{name}: the layout's shape {lay.shapes[name]} is not that of the bounds")
        out[name] = pool[lay[name]:lay.end(name)].reshape(lay.shapes[name])
    return out


def regions(lay):
    """[(region name, first element, one past the last)] in pool order.  The guard between two arrays is split in its middle:
    ``guard after <left>`` up to there, ``guard before <right>`` from there on."""
    out, at = [], 0
    for pos, name in enumerate(lay.names):
        split = at if pos == 0 else (at + lay[name]) // 2
        if pos:
            out.append((f"guard after {lay.names[pos - 1]}", at, split))
        out.append((f"guard before {name}", split, lay[name]))
        out.append((name, lay[name], lay.end(name)))
        at = lay.end(name)
    out.append((f"guard after {lay.names[-1]}", at, lay.length))
    return out


def diff(got_pool, want_pool, lay, nan_payloads_free=False):
    """None when the two pools hold the same bytes.  Otherwise a dict: ``region`` (an array's name, ``guard before <name>`` or
    ``guard after <name>``) of the FIRST differing element, ``offset`` (its pool index), ``index`` (array regions: the index
    into the array, (j, k, i) for a 3-D one, a member axis in front where stacked) or ``distance`` (guards: elements to the
    nearest cell of the array the guard is named after), ``got`` / ``want`` (the two bit patterns) and ``counts``: region ->
    differing elements.  ``nan_payloads_free``: inside ARRAYS a NaN equals any NaN (where a test plants one); guards stay bytes."""
    got, want = np.ascontiguousarray(got_pool), np.ascontiguousarray(want_pool)
    if got.dtype != lay.dtype or want.dtype != lay.dtype or got.shape != (lay.length,) or want.shape != (lay.length,):
        raise ValueError("diff needs two pools of the layout's dtype and length")
    u = _uint(lay.dtype)
    bad = got.view(u) != want.view(u)
    if nan_payloads_free:
        both_nan = np.isnan(got) & np.isnan(want)
        for name in lay.names:
            bad[lay[name]:lay.end(name)] &= ~both_nan[lay[name]:lay.end(name)]
    if not bad.any():
        return None
    e = int(np.argmax(bad))
    out = dict(offset=e, got=hex(int(got.view(u)[e])), want=hex(int(want.view(u)[e])), counts={})
    for name, first, end in regions(lay):
        n = int(np.count_nonzero(bad[first:end]))
        if n:
            out["counts"][name] = n
        if first <= e < end:
            out["region"] = name
            if name in lay:
                out["index"] = tuple(int(x) for x in np.unravel_index(e - first, lay.shapes[name]))
            else:
                out["distance"] = e - first + 1 if name.startswith("guard after") else end - e
    return out
