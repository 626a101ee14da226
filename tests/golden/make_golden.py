"""Regenerates tests/golden/ from the REFERENCE Fortran itself.

Run in the build container only (needs /root/reference and amdflang):

    python tests/golden/make_golden.py

It compiles the reference's module_configure.f90 + module_small_step_em.f90 from where they
lie into oracle/_ref/ (oracle/Makefile `ref`; nothing is copied into the repository), runs
`advance_mu_t` on this repository's seeded synthetic inputs and stores

* golden_small.npz, golden_small_shapes.npz
                       -- all 7 outputs, full arrays, of 16x8x16 (every flag combination)
                          and of the ragged / tile / one-level cases (flags none, specified);
                          split by shape (cases.GOLDEN_SMALL) so that no file passes 1 MiB
* golden_digests.json  -- sha256 of every input and output array of every case (incl. 64x40x64)
* extra_reference_digests.json -- sha256 of every array after the reference's call on the random
                          extra cases of tests/cases.py (extra_case), fp32 and fp64
* hard_inputs_digests.json -- sha256 of the 7 outputs (and of the 4 vertical metrics going in) of every
                          shape of cases.SHAPES plus a tall sub-tile, every flag combination, fp32 and fp64,
                          with the WRF-like metrics and each scalar set of tests/hard_inputs.py
* special_values_digests.json -- sha256, every NaN mapped to one bit pattern (cases.digest_canonical_nan), of the 7 outputs of
                          the regimes of tests/special_values.py on three small shapes, every flag combination, fp32 and
                          fp64; of every single plant on 37x5x11_ragged one digest over the 7 outputs

The reference ships no golden vectors of its own (its drivers diff against an absent
/data2/... directory), so these are the pinned known answers.
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import __graft_entry__ as g  # noqa: E402
import cases  # noqa: E402
import hard_inputs  # noqa: E402
import special_values  # noqa: E402


FULL_SHAPES = ("37x5x11_ragged", "130x3x7_tile", "70x1x9_onelevel")   # stored as full arrays


def main():
    oracle = g.load_oracle()
    oracle.build(ref=True)
    pkg = g.load_package()
    small, digests = {}, {}
    for shape in cases.SHAPES:
        for flag in cases.FLAG_COMBOS:
            for dtype in (np.float32, np.float64):
                key = f"{shape}/{flag}/{np.dtype(dtype).name}"
                p = cases.make_case(pkg, shape, flag, dtype)
                inputs = {n: cases.digest(a) for n, a in p.arrays.items()}
                oracle.ref_advance_mu_t(*p.args())
                digests[key] = {"bounds": list(p.bounds.as_tuple()), "inputs": inputs,
                                "outputs": {n: cases.digest(p.arrays[n]) for n in pkg.synth.FIELD_NAMES}}
                if shape == "16x8x16" or (shape in FULL_SHAPES and flag in ("none", "specified")):
                    for n in pkg.synth.OUTPUTS:
                        small[f"{key}/{n}"] = p.arrays[n]
    for name, shapes in cases.GOLDEN_SMALL.items():
        np.savez_compressed(HERE / name, **{k: v for k, v in small.items() if k.split("/")[0] in shapes})
    (HERE / "golden_digests.json").write_text(json.dumps(digests, indent=1, sort_keys=True))
    print(f"wrote {len(small)} arrays, {len(digests)} cases")
    extra_reference_digests(pkg, oracle)
    hard_inputs_digests(pkg, oracle)
    special_values_digests(pkg, oracle)


def extra_reference_digests(pkg, oracle):
    extra = {}
    for dtype in (np.float32, np.float64):
        recs = []
        for trial in range(cases.EXTRA_TRIALS):
            p = cases.extra_case(pkg, trial, dtype)
            oracle.ref_advance_mu_t(*p.args())
            recs.append({"bounds": list(p.bounds.as_tuple()),
                         "fields": {n: cases.digest(p.arrays[n]) for n in pkg.synth.FIELD_NAMES}})
        extra[np.dtype(dtype).name] = recs
    (HERE / "extra_reference_digests.json").write_text(json.dumps(extra, indent=1, sort_keys=True))
    print(f"wrote {sum(len(v) for v in extra.values())} extra cases")


def hard_inputs_digests(pkg, oracle):
    recs = {}
    for key in hard_inputs.hard_keys():
        shape, flag, dtname, sset = key.split("/")
        p = hard_inputs.hard_case(pkg, shape, flag, np.dtype(dtname), sset)
        metrics = {n: cases.digest(p.arrays[n]) for n in hard_inputs.RANK1}
        oracle.ref_advance_mu_t(*p.args())
        recs[key] = {"bounds": list(p.bounds.as_tuple()), "scalars": [p.rdx, p.rdy, p.dts, p.epssm], "metrics": metrics,
                     "outputs": {n: cases.digest(p.arrays[n]) for n in pkg.synth.OUTPUTS}}
    (HERE / "hard_inputs_digests.json").write_text(json.dumps(recs, indent=0, sort_keys=True))
    print(f"wrote {len(recs)} hard-input cases")


def special_values_digests(pkg, oracle):
    recs = {}
    for key in special_values.regime_keys():
        p = special_values.special_case(pkg, key)
        oracle.ref_advance_mu_t(*p.args())
        recs[key] = {"bounds": list(p.bounds.as_tuple()), "scalars": [p.rdx, p.rdy, p.dts, p.epssm], "seed": special_values.SEED,
                     "outputs": {n: cases.digest_canonical_nan(p.arrays[n]) for n in pkg.synth.OUTPUTS}}
    for key in special_values.plant_keys():
        p = special_values.special_case(pkg, key)
        oracle.ref_advance_mu_t(*p.args())
        canon = [special_values.canonical_nan(p.arrays[n]).view(np.uint8).ravel() for n in pkg.synth.OUTPUTS]
        recs[key] = {"outputs": cases.digest(np.concatenate(canon))}
    (HERE / "special_values_digests.json").write_text(json.dumps(recs, indent=0, sort_keys=True))
    print(f"wrote {len(recs)} special-value cases")


if __name__ == "__main__":
    if sys.argv[1:] == ["special_values"]:                   # this file alone; the others stay as they are
        _oracle = g.load_oracle()
        _oracle.build(ref=True)
        special_values_digests(g.load_package(), _oracle)
    else:
        main()
