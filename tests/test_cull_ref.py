"""The reference of tests/test_gpu_culls.py held to itself without a GPU: the rows it builds are what it says they are, and its judgement, run on a numpy fp32
restatement of the culls (cull_ref.emulate), finds no false reject, rejects beyond the padding and has teeth on the negative control - so that a failure of the
GPU test is the device's, not the judge's."""
import numpy as np

import cull_ref as ref
from hsr_env_amd import model as hm


def emulated_output(inp):
    w = inp["words"]
    out = np.zeros((len(w), ref.OUT_W), dtype=np.uint32)
    out[:, :6] = ref.emulate(w)
    pk = ((((w[:, 55].astype(np.uint64) + 0xFFFF) >> 16) << 16).astype(np.uint32)) | w[:, 6] | (w[:, 7] << 6) | (w[:, 8] << 12)
    back = (pk & 0xFFFF0000).astype(np.uint32)
    out[:, 6], out[:, 7] = pk, back
    out[:, 8] = (back.view(np.float32) + np.ascontiguousarray(w[:, 54]).view(np.float32)).view(np.uint32)
    out[:, 9], out[:, 10], out[:, 11] = pk & 63, (pk >> 6) & 63, (pk >> 12) & 3
    out[:, 12] = np.array([ref.SKIN], dtype=np.float32).view(np.uint32)[0]
    out[[i for i in range(len(out)) if ref.lane_off(i)]] = ref.SENTINEL
    return out


def test_rows_are_what_the_reference_says():
    inp = ref.all_inputs()
    facts, words = inp["facts"], inp["words"]
    assert 2000 <= inp["n_geo"] <= 6000 and len(words) % 64 == 0
    kinds = {f["kind"] for f in facts}
    assert {"box-box", "hull-box", "box-hull", "hull-hull", "cyl-box", "cyl-hull", "plane-box", "plane-hull", "plane-cyl"} <= kinds
    assert sum(f["kind"] in ("hull-hull", "cyl-box", "cyl-hull") for f in facts) <= 900
    fl = np.ascontiguousarray(words[inp["slot"][:inp["n_geo"]], 10:56]).view(np.float32).astype(np.float64)
    assert np.all(np.abs(fl[:, 0:3]) <= 2.0), "first shapes within +-2 m"
    for f, r in zip(facts, fl):
        # placement: the separation along u came out as asked, up to the fp32 rounding of a position within a few metres
        assert abs(f["gap"] - f["g"]) <= 1.5e-6, f
        assert f["dup"] >= abs(f["gap"]) - 1e-12
        if f["gap"] <= 0 and not f["plane"]:
            assert f["depth"] <= -f["gap"] + 1e-9, f      # u is one separating direction: no deeper than the overlap along it
        for o in (3, 24):                                  # the rounded matrices are rotations to fp32
            M = r[o:o + 9].reshape(3, 3)
            assert np.abs(M.T @ M - np.eye(3)).max() < 1e-6
    S = ref.shapes()
    assert S["plane"].type == hm.GEOM_PLANE and S["cyl"].type == hm.GEOM_CYLINDER and S["table"].type == hm.GEOM_BOX
    assert all(20 <= S[k].nvert <= 45 for k in ("wrist", "palm", "lprox", "ldist", "rdist"))


def test_judgement_on_the_fp32_restatement():
    inp = ref.all_inputs()
    out = emulated_output(inp)
    assert ref.check_lanes(out, inp) > 0
    geo, ctrl, pack = ref.split(out, inp)
    touch, near = ref.check_no_false_reject(geo, inp["facts"])
    n0, ns, frontier = ref.check_tightness(geo, inp["facts"])
    same, sphere = ref.check_chain_and_persistent_agree(geo, inp["facts"])
    counts = ref.check_control(ctrl, inp["facts"])
    worst, exact = ref.check_pack(pack, inp)
    print(f"touching {touch}, within skin {near}, tightness rows {n0} / {ns}, verdicts equal {same} / sphere only {sphere}, control {counts}, pack worst {worst:.6f}")
    assert touch >= 400 and near >= 2000 and n0 >= 200 and ns >= 50
    # the judge sees a cull that is too tight: one touching pair rejected is reported
    k = int(np.flatnonzero(ref.must_pass(inp["facts"])[0])[0])
    geo2 = geo.copy(); geo2[k, 3] = 0
    try:
        ref.check_no_false_reject(geo2, inp["facts"])
    except AssertionError:
        return
    raise AssertionError("a rejected touching pair went unnoticed")
