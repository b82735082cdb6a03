"""
CPU: what the GPU test of the one-kernel step with aux planes (tests/test_gpu_fused_aux.py) stands on -- the worker's
cases cover what they are meant to cover, its numpy boundary fill and oracle chain are sound (the chain reproduces the
reference's own step2ds.f golden), and the built library carries the new step2ds_kernel instantiations for gfx950.
"""
import importlib.util
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("fused_aux_worker", os.path.join(HERE, "fused_aux_worker.py"))
W = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(W)


def test_cases_cover_solvers_boundaries_limiters_orders():
    cs = W.cases()
    assert len({c.name for c in cs}) == len(cs) >= 30
    by_rp = {}
    for c in cs:
        by_rp.setdefault((c.rp, c.mcapa > 0), []).append(c)
    for rp in (W.RP_VC_ACOUSTICS, W.RP_VC_ADVECTION, W.RP_PSYSTEM):
        assert (rp, False) in by_rp
    for rp in (W.RP_ACOUSTICS, W.RP_ADVECTION, W.RP_EULER5, W.RP_SHALLOW, W.RP_VC_ACOUSTICS):
        assert (rp, True) in by_rp
    assert {t for c in cs for t in c.bc if t >= 0} == {W.CST, W.OUT, W.PER, W.REF}
    vc = by_rp[(W.RP_VC_ACOUSTICS, False)]
    assert {m for c in vc for m in c.mthlim} == set(range(6)) and {c.order for c in vc} == {1, 2}
    assert {(60, 12), (61, 13), (59, 11), (300, 5), (3, 90), (300, 100)} <= {(c.mx, c.my) for c in vc}
    for c in cs:
        assert 10 <= c.steps <= 100 or c.ghosts, c.name
        assert (c.bc[0] == W.PER) == (c.bc[1] == W.PER) and (c.bc[2] == W.PER) == (c.bc[3] == W.PER), c.name
        if c.mcapa:
            assert c.aux[c.mcapa - 1].min() >= 0.5, c.name
        assert c.q.flags.f_contiguous and c.aux.flags.f_contiguous and np.isfinite(c.q).all()


def test_fill_ghosts_is_y_of_x():
    rng = np.random.default_rng(0)
    q = np.asfortranarray(rng.standard_normal((3, 9, 8)))
    cst = np.zeros((4, 8))
    cst[3, :3] = [7.0, 8.0, 9.0]
    f = W.fill_ghosts(q.copy("F"), [W.PER, W.PER, W.REF, W.CST], cst)
    assert np.array_equal(f[:, 2:-2, 2:-2], q[:, 2:-2, 2:-2])
    assert np.array_equal(f[:, :2, 2:-2], q[:, 5:7, 2:-2]) and np.array_equal(f[:, 7:, 2:-2], q[:, 2:4, 2:-2])
    # reflecting in y: the mirror row of the x-filled array, the y momentum negated; x ghost columns included
    assert np.array_equal(f[0, :, 0], f[0, :, 3]) and np.array_equal(f[2, :, 1], -f[2, :, 2]) and np.array_equal(f[1, :, 0], f[1, :, 3])
    assert (f[0, :, 6:] == 7.0).all() and (f[2, :, 6:] == 9.0).all()
    o = W.fill_ghosts(q.copy("F"), [W.OUT, W.REF, -1, -1], cst)
    assert np.array_equal(o[:, 0, :], q[:, 2, :]) and np.array_equal(o[1, 8, :], -q[1, 5, :]) and np.array_equal(o[0, 7, :], q[0, 6, :])
    assert np.array_equal(o[:, 2:-2, :], q[:, 2:-2, :])


def test_oracle_chain_starts_from_the_reference_golden(coracle):
    """the x pass of the chained oracle step on the golden's input is the reference's step2ds.f result (ids = 1)"""
    c = {k.name: k for k in W.cases()}["golden_capa"]
    z = np.load(os.path.join(HERE, "golden", "ref_step2ds_capa.npz"), allow_pickle=False)
    qx = c.q.copy("F")
    _, cfl = coracle.step2ds(c.rp, c.par, max(c.mx, c.my), 2, c.mx, c.my, c.q.copy("F"), qx, c.aux, c.dx, c.dy, c.dt,
                             c.method(), np.array(c.mthlim, dtype=np.int32), 1)
    assert np.array_equal(qx, z["q_ids1"]) and cfl == float(z["cfl_ids1"])
    full, cfls = W.oracle_run(coracle, c)
    assert len(cfls) == 1 and cfls[0] >= cfl and not np.array_equal(full, qx[:, 2:-2, 2:-2])


def test_oracle_runs_stay_within_the_cfl_limit(coracle):
    """the cases' fixed time steps keep every step's Courant number inside (0, 1) and the states finite"""
    for c in W.cases():
        if c.mx * c.my > 130 * 75 or c.steps > 30:
            continue                                   # the large grids run on the GPU side only
        q, cfls = W.oracle_run(coracle, c)
        assert np.isfinite(q).all() and 0.0 < max(cfls) < 1.0, (c.name, max(cfls))


def test_library_holds_the_new_instantiations():
    """hipcc --offload-arch=gfx950 built step2ds_kernel for the aux-carrying solvers and with a capacity function, in the
    three arithmetic modes (the kernel names are in the code object's symbol table, inside the shared library)"""
    from pyclaw_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "run __graft_entry__.build() first"
    blob = open(_lib.LIB_PATH, "rb").read()
    for ns in (b"5exact", b"4fast", b"6strict"):
        for rp, fw in ((b"13VcAcoustics2DE", b"Lb0E"), (b"13VcAdvection2DE", b"Lb0E"), (b"12FwaveElasticILi3EEE", b"Lb1E")):
            for capa in (b"Lb0E", b"Lb1E"):
                assert b"_ZN3pcl" + ns + b"14step2ds_kernelINS0_" + rp + fw + b"Lb0E" + capa + b"EEv" in blob, (ns, rp, capa)
        for rp in (b"6Euler5E", b"11Acoustics2DE", b"11Advection2DE", b"9Shallow2DE"):
            assert b"_ZN3pcl" + ns + b"14step2ds_kernelINS0_" + rp + b"Lb0ELb0ELb1EEEv" in blob, (ns, rp)
