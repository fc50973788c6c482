"""sageicp_graph_info_from_quality (include/sageicp.h "robust pose graph") on the CPU: a closure edge's
information from the quality report at the closed pose.

  * the tangent relation derived on its own: closed <- exp(xi) closed moves z = poses[i]^-1 closed to z exp(eta) with
    eta = Ad(closed^-1) xi whatever poses[i] — closed^-1 exp(xi) closed = exp(Ad(closed^-1) xi) —, in np.longdouble with
    posegraphref's SE(3);
  * the library against info = gain Ad(closed)^T (JTJ / s2) Ad(closed), symmetrised, restated in np.longdouble: allowed four
    times the fp64 restatement's own error (closureref's rule), with one ulp of the largest entry as the floor;
  * the result goes through sageicp_graph_edge_from_closed's check; every refusal writes nothing; a report at UTM
    coordinates is refused or positive definite, never garbled.
The reports are made here: JTJ = sum w J^T J with J = [I | -hat(s)] over points s around the closed pose, as the header
states it."""
import ctypes

import numpy as np
import pytest

import posegraphref as pg

DP = ctypes.POINTER(ctypes.c_double)


def _pose(seed, t):
    rng = np.random.default_rng(seed)
    q = rng.normal(size=4)
    return np.concatenate([q / np.linalg.norm(q), np.asarray(t, dtype=np.float64)])


def _report(sage, seed, centre, n=400, spread=20.0):
    """a Quality record with the sums of n pairs around `centre`"""
    rng = np.random.default_rng(seed)
    s = np.asarray(centre) + spread * rng.normal(size=(n, 3)) * np.array([1.0, 1.0, 0.2])
    w = rng.uniform(0.2, 1.0, size=n)
    r = 0.05 * rng.normal(size=(n, 3))
    J = np.zeros((n, 3, 6))
    J[:, :, :3] = np.eye(3)
    J[:, :, 3:] = -pg._hat(s)
    q = sage.Quality()
    q.JTJ[:] = list(np.einsum("n,nki,nkj->ij", w, J, J).reshape(-1))
    q.sum_w_r2 = float((w * (r * r).sum(axis=1)).sum())
    q.n_pairs, q.n_queries = n, n
    q.valid, q.covariance_valid = 1, 1
    return q


def _restated(q, closed, gain, dtype):
    f = np.dtype(dtype).type
    M = np.array(q.JTJ[:], dtype=np.float64).reshape(6, 6).astype(dtype)
    s2 = f(q.sum_w_r2) / (f(3) * f(q.n_pairs) - f(6))
    c = np.asarray(closed, dtype=np.float64).astype(dtype)[None]
    c[:, :4] /= np.sqrt((c[:, :4] * c[:, :4]).sum())
    Ad = pg.vadjoint(c)[0]
    O = f(gain) * (Ad.T @ (M / s2) @ Ad)
    return (O + O.T) / f(2)


def _call(sage, q, closed, gain):
    out = np.full(36, 7.25)
    rc = sage.lib().sageicp_graph_info_from_quality(None if q is None else ctypes.byref(q),
                                                    None if closed is None else np.ascontiguousarray(closed, dtype=np.float64).ctypes.data_as(DP),
                                                    float(gain), out.ctypes.data_as(DP))
    return rc, out


def test_the_tangent_relation():
    ld = np.longdouble
    closed = _pose(1, [30.0, -12.0, 2.0]).astype(ld)[None]
    closed[:, :4] /= np.sqrt((closed[:, :4] ** 2).sum())
    Ad_inv = pg.vadjoint(pg.vinv(closed))[0]
    worst = 0.0
    for p_seed in (2, 3):                                        # two different poses[i]: the relation does not depend on it
        p = _pose(p_seed, [5.0 * p_seed, 40.0, -1.0]).astype(ld)[None]
        p[:, :4] /= np.sqrt((p[:, :4] ** 2).sum())
        z = pg.vbetween(p, closed)
        for k in range(6):
            xi = np.zeros((1, 6), dtype=ld)
            xi[0, k] = ld(1e-6)
            z2 = pg.vbetween(p, pg.vmul(pg.vexp(xi), closed))
            eta = pg.vlog(pg.vmul(pg.vinv(z), z2))[0]
            want = Ad_inv @ xi[0]
            err = float(np.abs(eta - want).max())
            worst = max(worst, err / float(np.abs(want).max()))
            # to second order: |xi| of the step itself
            assert err <= 1e-6 * float(np.abs(want).max()), (k, err)
    print("eta against Ad(closed^-1) xi at |xi| = 1e-6: relative difference %.3g" % worst)
    # and NOT the identity: at 30 m the adjoint moves a rotation's xi by metres
    assert np.abs(Ad_inv - np.eye(6)).max() > 1.0


@pytest.mark.parametrize("gain", [1.0, 0.01])
def test_against_the_restatement(sage, gain):
    poses = np.array([_pose(7, [1.0, 2.0, 0.5]), _pose(8, [20.0, 5.0, 0.0])])
    for seed, t in ((11, [0.0, 0.0, 0.0]), (12, [30.0, -12.0, 2.0]), (13, [-150.0, 80.0, 5.0])):
        closed = _pose(seed, t)
        closed[:4] *= 1.0 + 1e-9                                 # (a quaternion as a registration returns it: unit to rounding)
        q = _report(sage, seed, t)
        info = sage.graph_edge_info(q, closed, gain)
        ext = _restated(q, closed, gain, np.longdouble)
        own = float(np.abs(_restated(q, closed, gain, np.float64).astype(np.longdouble) - ext).max())
        got = float(np.abs(info.astype(np.longdouble) - ext).max())
        floor = float(np.abs(ext).max()) * 2.0 ** -52
        print("closed at %s, gain %g: the fp64 restatement %.3g from the extended one, the library %.3g (allowed %.3g); largest entry %.3g"
              % (t, gain, own, got, 4.0 * max(own, floor), float(np.abs(ext).max())))
        assert got <= 4.0 * max(own, floor)
        assert info.shape == (6, 6) and info.tobytes() == info.T.copy().tobytes()           # symmetric to the bit
        # the optimiser's own check takes it
        e = sage.graph_edge(poses, 0, 1, closed, info)
        assert np.array(e.info[:]).tobytes() == info.tobytes()
        # the quadratic form is the report's: eta^T info eta = gain xi^T (JTJ / s2) xi with xi = Ad(closed) eta
        rng = np.random.default_rng(seed)
        eta = rng.normal(size=6)
        c = closed.copy()
        c[:4] /= np.linalg.norm(c[:4])
        xi = pg.vadjoint(c[None])[0] @ eta
        s2 = q.sum_w_r2 / (3.0 * q.n_pairs - 6.0)
        want = gain * xi @ (np.array(q.JTJ[:]).reshape(6, 6) / s2) @ xi
        assert eta @ info @ eta == pytest.approx(want, rel=1e-9)


def test_every_refusal_writes_nothing(sage):
    closed = _pose(12, [30.0, -12.0, 2.0])
    good = _report(sage, 12, closed[4:])
    assert _call(sage, good, closed, 1.0)[0] == 0

    def changed(**kw):
        q = sage.Quality.from_buffer_copy(good)
        for k, v in kw.items():
            if k == "JTJ":
                q.JTJ[:] = list(np.asarray(v, dtype=np.float64).reshape(-1))
            else:
                setattr(q, k, v)
        return q

    M = np.array(good.JTJ[:]).reshape(6, 6)
    cases = [("q NULL", None, closed, 1.0), ("closed NULL", good, None, 1.0),
             ("no valid covariance", changed(covariance_valid=0), closed, 1.0),
             ("s2 is 0", changed(sum_w_r2=0.0), closed, 1.0), ("s2 below 0", changed(sum_w_r2=-1.0), closed, 1.0),
             ("two pairs", changed(n_pairs=2), closed, 1.0), ("no pairs", changed(n_pairs=0), closed, 1.0),
             ("gain 0", good, closed, 0.0), ("gain below 0", good, closed, -1.0),
             ("a zero quaternion", good, np.array([0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0]), 1.0),
             ("JTJ zero", changed(JTJ=np.zeros((6, 6))), closed, 1.0), ("JTJ indefinite", changed(JTJ=-M), closed, 1.0)]
    for bad in (np.nan, np.inf, -np.inf):
        cases.append(("gain %s" % bad, good, closed, bad))
        cases.append(("sum_w_r2 %s" % bad, changed(sum_w_r2=bad), closed, 1.0))
        B = M.copy()
        B[2, 4] = B[4, 2] = bad
        cases.append(("JTJ %s" % bad, changed(JTJ=B), closed, 1.0))
        for col in (0, 3, 5):
            c = closed.copy()
            c[col] = bad
            cases.append(("closed[%d] %s" % (col, bad), good, c, 1.0))
    for what, q, c, gain in cases:
        rc, out = _call(sage, q, c, gain)
        assert rc == sage.ERR_INVALID, what
        assert (out == 7.25).all(), what
    with pytest.raises(ValueError):
        sage.graph_edge_info(good.JTJ, closed)
    with pytest.raises(sage.SageIcpError):
        sage.graph_edge_info(changed(covariance_valid=0), closed)


def test_a_report_at_utm_is_refused_or_positive_definite(sage):
    """the sums of a 20 m scene at (5e5, 5e6): JTJ's rotation block is 1e13 times its translation block and the report's own
    covariance flag is what tells a caller to register in a local frame; whatever the flag, the conversion either refuses
    or returns a matrix the optimiser accepts"""
    utm = np.array([5.0e5, 5.0e6, 0.0])
    poses = np.array([_pose(7, utm + [1.0, 2.0, 0.5]), _pose(8, utm + [20.0, 5.0, 0.0])])
    seen = set()
    for seed in range(20, 30):
        closed = _pose(seed, utm + [30.0, -12.0, 2.0])
        q = _report(sage, seed, closed[4:], spread=20.0 if seed % 2 else 2.0)
        rc, out = _call(sage, q, closed, 1.0)
        seen.add(rc)
        if rc != 0:
            assert rc == sage.ERR_INVALID and (out == 7.25).all()
            continue
        info = out.reshape(6, 6)
        assert np.isfinite(info).all() and info.tobytes() == info.T.copy().tobytes()
        np.linalg.cholesky(info)                                 # (raises if it is not positive definite)
        sage.graph_edge(poses, 0, 1, closed, info)
    print("at UTM: return codes seen %s" % sorted(seen))
