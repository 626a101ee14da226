"""Randomised geometry campaign for everything written since tests/test_gpu_12_random.py: the ensemble launch, the cyclic
refresh, the boundary-zone update, the flux averages, the stage bracket, the ensemble moments, the field statistics and the
composition of all of them on the handles.  tests/random_geometry.py draws the cases -- small on purpose, odd row lengths, every
16-byte phase, member strides off 16 bytes, tiles clipped in one direction only, kms = -2 pads, and about one in twenty large
enough for a launch to go round its grid -- and plays each family's script twice: through the numpy references (and the C oracle
for a sweep) and through the library on the device.  Every array of a call, inputs included, is compared whole and as bytes;
cells the calls of a case do not read hold NaN with payloads of their own -- in the sweep families too, where the 26 arrays of
synth.make_patch are poisoned outside the read masks (tests/special_values.py and, on the handles, the union over the calls).  Seeded: a failure names seed, case number and bounds;
AMT_GEOM_CASES=N and AMT_GEOM_SEED=S run other campaigns.  tests/test_random_geometry_cpu.py shows without a GPU that these
cases catch the bugs they are drawn for."""
import ctypes
import json
import time

import numpy as np
import pytest

import random_geometry as G
import stage_ref as ST
import sumflux_ref as SF

pytestmark = pytest.mark.gpu

CYCLIC_ORDER = ("u", "u_1", "v", "v_1", "t_1", "muu", "muv", "msfuy", "msfvx_inv")
NAMES13 = SF.ACCUMULATORS + SF.INPUTS
STATS_KEYS = ("count", "n_nan", "n_inf", "first_nonfinite", "min", "max", "max_abs", "sum")
DIFF_KEYS = ("count", "n_diff", "first_diff", "max_abs_diff")


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


class DeviceOps:
    """The library in the place of the references: upload, ONE call (or, for the handles, one stage), download -- in place on
    the numpy arrays the script hands over, every array of the call."""

    def __init__(self, pkg, torch):
        self.pkg, self.torch, self.L = pkg, torch, pkg.load_library()
        self.skipped = 0                           # march calls that ended with status 3: no march shape for the level count

    def _up(self, arrays):
        dev = {n: self.torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0") for n, a in arrays.items()}
        self.torch.cuda.synchronize()
        return dev

    def _down(self, dev, arrays):
        self.torch.cuda.synchronize()
        for n, a in arrays.items():
            a[...] = dev[n].cpu().numpy()

    def _cfg(self, case):
        return self.pkg.GridConfig(*[bool(x) for x in case.flags])

    def sweep(self, stacked, case, variant, scalars):
        pkg, S = self.pkg, self.pkg.synth
        dev = self._up(stacked)
        status = 0
        try:
            # one case in five through the register flavour of the march kernel, as tests/test_gpu_12_random.py does
            self.L.amt_march_force_shape(0, 0, 0, -1, 0 if case.params["register"] else 1, 0, 0)
            pkg.advance_mu_t_ensemble(*S.Patch(case.bounds, self._cfg(case), dev, *scalars[:4]).args(), members=case.members, variant=variant)
        except pkg.AmtError as e:
            if not (variant == pkg.VARIANT_MARCH and e.status == 3):
                raise AssertionError(f"{case.what()}: {e}")
            status = 3
            self.skipped += 1
        finally:
            self.L.amt_march_force_shape(0, 0, 0, -1, 1, 0, 0)
        self._down(dev, stacked)
        return status

    def cyclic(self, arrays, case):
        dev = self._up(arrays)
        self.pkg.cyclic_fill(*[dev[n] for n in CYCLIC_ORDER], self._cfg(case), *case.bounds.as_tuple(), axes=case.params["axes"],
                             members=case.members)
        self._down(dev, arrays)

    def spec_bdy(self, arrays, case):
        dev = self._up(arrays)
        self.pkg.spec_bdy_update(*[dev[n] for n in G.BDY_NAMES], case.params["dts"], self._cfg(case), *case.bounds.as_tuple(),
                                 members=case.members)
        self._down(dev, arrays)

    def sumflux(self, acc, inp, case, iteration, n):
        dev = self._up(dict(acc, **inp))
        self.pkg.sumflux(*[dev[name] for name in NAMES13], iteration, n, *case.bounds.as_tuple(), members=case.members)
        self._down(dev, dict(acc, **inp))

    def prep(self, a, case, rk_step):
        dev = self._up(a)
        self.pkg.stage_prep(*[dev[n] for n in ST.PREP], rk_step, *case.bounds.as_tuple(), members=case.members)
        self._down(dev, a)

    def finish(self, a, case, n, dts, with_h):
        dev = self._up(a)
        self.pkg.stage_finish(*[dev[x] for x in ST.FINISH], dts, n, dev["h_diabatic"] if with_h else None, *case.bounds.as_tuple(),
                              members=case.members)
        self._down(dev, a)

    def moments(self, a, outs, case):
        dev = self._up(dict(outs, a=a))
        self.pkg.diag.moments(dev["a"], extents=G.box_extents(case), box=G.box_of(case), want=(), out={n: dev[n] for n in outs})
        self._down(dev, dict(outs, a=a))

    def stats(self, a, case):
        dev = self._up(dict(a=a))
        got = self.pkg.diag.field_stats(dev["a"], stacked=True, extents=G.box_extents(case), box=G.box_of(case))
        self._down(dev, dict(a=a))
        return [{k: getattr(r, k) for k in STATS_KEYS} for r in got]

    def compare(self, a, bb, case):
        dev = self._up(dict(a=a, b=bb))
        got = self.pkg.diag.compare(dev["a"], dev["b"], stacked=True, extents=G.box_extents(case), box=G.box_of(case))
        self._down(dev, dict(a=a, b=bb))
        return [{k: getattr(r, k) for k in DIFF_KEYS} for r in got]

    def stage_on_handle(self, case, fields, extras, acc, scalars):
        """amt_domain_wrap or Ensemble.wrap over the caller's arrays, the case's settings, then stage_prep, the stepped sweeps
        with new exchanged inputs in front of each, stage_finish."""
        from wrf_model_cuda_sample_amd import lib
        pkg, torch, S, p, b = self.pkg, self.torch, self.pkg.synth, case.params, case.bounds
        dev, dev_x, dev_acc = self._up(fields), self._up(extras), self._up(acc)
        stream = torch.cuda.Stream()
        if p["kind"] == "ensemble":
            h = pkg.Ensemble.wrap(dev, b, self._cfg(case), stream=stream)
        else:
            h = lib.ResidentHandle()
            h.L, h.handle = self.L, ctypes.c_void_p()
            ptrs = (ctypes.c_void_p * len(S.FIELD_NAMES))(*[dev[n].data_ptr() for n in S.FIELD_NAMES])
            lib.check(self.L.amt_domain_wrap(ctypes.byref(h.handle), np.dtype(case.dtype).itemsize, *self._cfg(case).as_ints(),
                                             *b.as_tuple(), ptrs, ctypes.c_void_p(stream.cuda_stream)))
        try:
            h.set_scalars(*scalars[:4])
            if p["axes"]:
                h.set_cyclic(p["axes"])
            if p["spec_bdy"]:
                h.set_spec_bdy(True)
            if p["sumflux"]:
                h.set_sumflux(p["sumflux"], *[dev_acc[n] for n in SF.ACCUMULATORS])
            if p["stage"]:
                h.set_stage(True, *[dev_x[n] for n in ST.EXTRAS])
                h.stage_prep(p["rk_step"])
            scratch = {n: a.copy() for n, a in fields.items()}
            for s in range(p["sweeps"]):
                G.refresh_exchanged(case, pkg, scratch, scalars, s)
                h.sync()
                for n in S.EXCHANGED_INPUTS:
                    if n != "t_1":
                        dev[n].copy_(torch.from_numpy(scratch[n]))
                torch.cuda.synchronize()
                h.step(1)
            if p["stage"]:
                h.stage_finish(p["sweeps"], dev_x["h_diabatic"] if p["with_h"] else None)
            h.sync()
        finally:
            h.close()
        self._down(dev, fields)
        self._down(dev_x, extras)
        self._down(dev_acc, acc)


def _play(case, dev_ops, ref_ops, pkg):
    """The case on the device against the case through the references; (march ran, column ran) for the ensemble family."""
    got = G.run(case, dev_ops, pkg)
    bad = G.first_difference(case, got, G.run(case, ref_ops, pkg))
    assert bad is None, bad
    return {label: arrays is not None for label, arrays in got}


@pytest.mark.parametrize("family", G.FAMILIES)
def test_random_geometries_match_the_references(pkg, oracle, torch_mod, family):
    dev_ops, ref_ops = DeviceOps(pkg, torch_mod), G.RefOps(pkg, oracle)
    count = G.N_CASES[family]
    ran, t_start = {}, time.time()
    strides = 0
    for case in G.cases(family):
        for label, done in _play(case, dev_ops, ref_ops, pkg).items():
            ran[label] = ran.get(label, 0) + int(done)
        strides += int(G.grid_stride(case))
    summary = {"family": family, "seed": G.SEED, "cases": count, "wall_s": round(time.time() - t_start, 2), "ran": ran,
               "march_status_3": dev_ops.skipped, "grid_stride_cases": strides, "failures": 0}
    print("random geometry campaign:", json.dumps(summary))
    if family == "ensemble":                                       # the shares tests/test_gpu_12_random.py asks for
        assert ran["march"] >= count * 0.8 and ran["column"] >= count * 0.95, ran


# Cases to keep, written as (family, bounds in the order of synth.INT_NAMES, flags, dtype, members, parameters): what a campaign
# has found goes here with its seed and number.  The first entries are the three geometries no hand-picked test had before the
# campaign existed: a tile that starts at an odd memory column of an odd-length row below a kms = -2 pad; three members whose
# stride is off 16 bytes; a tile with jte == jde and ite < ide.
REGRESSIONS = [
    ("stage", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 2, 5, 1, 4), (0, 0, 0), np.float64, 1, dict(rk_step=2, n=3, with_h=True, dts=1.7)),
    ("stage", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 2, 5, 1, 4), (0, 0, 0), np.float32, 3, dict(rk_step=1, n=2, with_h=False, dts=0.3)),
    ("sumflux", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 2, 5, 1, 4), (0, 0, 0), np.float32, 3, dict(n=3)),
    ("sumflux", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 2, 6, 1, 4), (0, 0, 0), np.float64, 3, dict(n=2)),
    ("stage", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 2, 6, 1, 4), (0, 0, 0), np.float64, 3, dict(rk_step=3, n=4, with_h=True, dts=2.0)),
    ("spec_bdy", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 2, 6, 1, 4), (0, 1, 0), np.float32, 3, dict(dts=2.0)),
    ("cyclic", (1, 12, 1, 6, 4, -2, 14, 0, 6, -2, 4, 3, 9, 1, 6, 1, 4), (1, 0, 0), np.float32, 3, dict(axes=2)),
    ("ensemble", (1, 12, 1, 6, 5, -2, 14, 0, 6, -2, 5, 3, 9, 2, 6, 1, 5), (0, 1, 0), np.float64, 3, dict(register=False)),
]


HAND_WRITTEN = 8                                                   # the entries above; found cases follow them


@pytest.mark.parametrize("kept", range(len(REGRESSIONS)))
def test_cases_to_keep(pkg, oracle, torch_mod, kept):
    family, bounds, flags, dtype, members, params = REGRESSIONS[kept]
    b = pkg.synth.Bounds(*bounds)
    case = G.Case(family, kept, 0, b, flags, dtype, members, False, dict(params))
    if kept < HAND_WRITTEN:                                        # what those entries are there for; a found case is as it was found
        assert b.idim % 2 == 1 and (b.its - b.ims) % 2 == 1 and b.kms == -2
        assert members == 1 or G.member_stride_off_16(case)
    ran = _play(case, DeviceOps(pkg, torch_mod), G.RefOps(pkg, oracle), pkg)
    assert all(done for label, done in ran.items() if label != "march"), ran       # (march: no shape for some level counts)
