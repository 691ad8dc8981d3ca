"""GPU parity of the block table's endomorphism split (msm_joint.hip GLV,
joint_horner.hip k_joint_horner2_glv / k_joint_finish_glv).

Contexts made here run with KZGX_FIXED_JOINT_GLV=1; every output is compared
exactly with the oracle's naive per-term MSM (corc.msm_naive) and with what a
context created under KZGX_FIXED_JOINT_GLV=0 -- the 254 / 255-plane path --
computes for the same call.  The variable is read once at context creation,
so that context lives in one fresh child process (this file run as a script),
which runs every case once and hands back its outputs.

Forced small blocks (g = 2, 3, 5) build at once; n covers one point, a whole
block, a block and a point, and a padded partial third block; batch 65
crosses a workgroup of the finish kernel and of stage 2's eight groups.
tests/test_joint_glv_model.py is the model the kernels follow; the device's
split is compared with it through kzgx_debug_joint_glv."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":  # the child process: the paths tests/conftest.py gives the suite
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _sub in ("oracle", os.path.join("kzg-commitments_amd", "python"), "tests"):
        sys.path.insert(0, os.path.join(_root, _sub))

import kzg_ref as K

pytestmark = pytest.mark.gpu

CURVES = [("BN254", K.BN254), ("BLS12381", K.BLS12381)]
GS = (2, 3, 5)
BATCHES = (1, 3, 65)
C_REQ = 8
N_T = 16  # tabled points: 2 g + 3 <= 13 of them are used


def limbs(vals):
    import corc
    return corc.ints_to_limbs(vals, 4)


def pt(curve, row, inf):
    import corc
    return None if inf else corc.array_to_points(curve, row[None, :])[0]


def edge_scalars(C):
    from test_joint_glv_model import edge_scalars as model_edges
    return model_edges(C)  # 0, 1, 2, 3, r - 1, r - 2, lambda, lambda +- 1, r - lambda, (r +- 1) / 2, 2^253, lambda^2


def rows_for(C, g, n, batch):
    """batch rows of n scalars: seeded random, the edge scalars moving through the blocks, one all-equal row"""
    edges = edge_scalars(C)
    rows = []
    for b in range(batch):
        row = K.random_scalars(C, n, seed=9000 + 100 * g + 10 * n + b)
        for j in range(min(n, 3)):
            row[(j + b) % n] = edges[(3 * b + j) % len(edges)]
        rows.append(row)
    if batch > 1:
        rows[1] = [edges[(g + n) % len(edges)]] * n  # every point on one edge scalar
    if batch > 2:
        rows[2] = [0] * n  # O through exact additions: S_1 = -phi(S_2)
    return rows


def cases(C):
    """(key, tau, g, ranges, n, batch, rows), the same list in this process and in the child"""
    out = []
    tau = K.default_tau(C)
    for g in GS:
        for n in (1, g, g + 1, 2 * g + 3):
            for batch in BATCHES:
                out.append(("g%d_n%d_b%d" % (g, n, batch), tau, g, 0, n, batch, rows_for(C, g, n, batch)))
    out.append(("ranges2", tau, 3, 2, 9, 3, rows_for(C, 3, 9, 3)))
    # degenerate SRS, tau = 1: every point is G, entries at infinity (the INF accumulation), and the plane sums
    # meet equal and opposite operands
    rows = rows_for(C, 5, 13, 3)
    rows[0][0], rows[0][1] = 12345, C.r - 12345
    out.append(("tau1", 1, 5, 0, 13, 3, rows))
    return out


def run_cases(name, C, oracle=None):
    """every case through one context per (tau, g): {key: (out, inf)}; with oracle, also checked against it"""
    import kzgx
    res, srs = {}, {}
    ctx, built = None, None
    try:
        for key, tau, g, ranges, n, batch, rows in cases(C):
            if built != (tau, g):
                if ctx:
                    ctx.close()
                ctx = kzgx.Context(name)
                ctx.gen_srs(tau, N_T)
                ctx.set_fixed_joint(g)
                ctx.set_fixed_base(C_REQ, N_T)
                assert ctx.fixed_joint_info()[0] == g
                built = (tau, g)
            ctx.set_fixed_joint_ranges(ranges)
            SB = np.concatenate([limbs(r) for r in rows])
            out, inf = ctx.msm_batch(SB, n, batch)
            res[key] = (out, inf)
            if oracle is not None:
                if tau not in srs:
                    srs[tau] = oracle.gen_srs(name, tau, N_T)
                for b in range(batch):
                    assert pt(name, out[b], inf[b]) == oracle.msm_naive(name, srs[tau][:n], limbs(rows[b])), (key, b)
    finally:
        if ctx:
            ctx.close()
    return res


@pytest.fixture(scope="module")
def glv_env():
    old = os.environ.get("KZGX_FIXED_JOINT_GLV")
    os.environ["KZGX_FIXED_JOINT_GLV"] = "1"
    yield
    if old is None:
        del os.environ["KZGX_FIXED_JOINT_GLV"]
    else:
        os.environ["KZGX_FIXED_JOINT_GLV"] = old


@pytest.fixture(scope="module")
def unsplit(tmp_path_factory):
    """{curve: {key: (out, inf)}} of the KZGX_FIXED_JOINT_GLV=0 path, from one fresh child process"""
    path = str(tmp_path_factory.mktemp("glv") / "unsplit.npz")
    env = dict(os.environ, KZGX_FIXED_JOINT_GLV="0")
    subprocess.run([sys.executable, os.path.abspath(__file__), path], check=True, env=env, timeout=300)
    z = np.load(path)
    return {name: {k[len(name) + 1:-4]: (z[k], z[k[:-4] + ":inf"]) for k in z.files
                   if k.startswith(name + ":") and k.endswith(":out")} for name, _ in CURVES}


@pytest.mark.parametrize("name,C", CURVES)
def test_split_matches_naive_and_unsplit(name, C, glv_env, unsplit, oracle_c):
    got = run_cases(name, C, oracle_c)
    ref = unsplit[name]
    assert set(got) == set(ref) and len(got) == len(GS) * 4 * len(BATCHES) + 2
    for key, (out, inf) in got.items():
        assert (out == ref[key][0]).all() and (inf == ref[key][1]).all(), key
    assert got["g5_n13_b3"][1][2] and got["tau1"][1][2]  # the all-zero rows are at infinity


@pytest.mark.parametrize("name,C", CURVES)
def test_device_split_is_the_models(name, C, glv_env):
    import kzgx
    from test_joint_glv_model import boundary_scalars, split
    sc = edge_scalars(C) + [C.r, C.r + 5, (1 << 256) - 1] + boundary_scalars(C) + K.random_scalars(C, 200, seed=77)
    S = np.ascontiguousarray(np.array([[(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)] for v in sc], dtype=np.uint32))
    out = np.zeros((len(sc), 9), dtype=np.uint32)
    ctx = kzgx.Context(name)
    try:
        fn = kzgx.lib().kzgx_debug_joint_glv
        fn.restype = ctypes.c_int
        fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
        assert fn(ctx.h, S.ctypes.data, len(sc), out.ctypes.data) == 0
    finally:
        ctx.close()
    for i, v in enumerate(sc):
        k1, k2 = split(C, v)
        got = [sum(int(out[i, 4 * h + q]) << (32 * q) for q in range(4)) for h in (0, 1)]
        assert got == [abs(k1), abs(k2)] and int(out[i, 8]) == (k1 < 0) | ((k2 < 0) << 1), (i, hex(v))


@pytest.mark.parametrize("name,C", CURVES)
def test_two_streams(name, C, glv_env, oracle_c):
    """two calls enqueued on two streams of one context, a synchronize, then the check"""
    import kzgx
    import torch
    dev = torch.device("cuda", 0)
    g, n, batch = 5, 13, 65
    tau = K.default_tau(C)
    ctx = kzgx.Context(name)
    try:
        ctx.gen_srs(tau, N_T)
        ctx.set_fixed_joint(g)
        ctx.set_fixed_base(C_REQ, N_T)
        rows = [rows_for(C, g, n, batch), rows_for(C, g, n - 1, batch)]
        ns = [n, n - 1]
        d_in = [torch.from_numpy(np.concatenate([limbs(r) for r in rs]).view(np.int64)).to(dev) for rs in rows]
        d_out = [torch.zeros((batch, 2 * ctx.w64), dtype=torch.int64, device=dev) for _ in rows]
        d_inf = [torch.zeros((batch,), dtype=torch.int32, device=dev) for _ in rows]
        streams = [torch.cuda.Stream(device=dev) for _ in rows]
        torch.cuda.synchronize(dev)
        for i in range(2):
            ctx.msm_batch_device(d_in[i].data_ptr(), ns[i], batch, ns[i], d_out[i].data_ptr(), d_inf[i].data_ptr(),
                                 streams[i].cuda_stream)
        torch.cuda.synchronize(dev)
        srs = oracle_c.gen_srs(name, tau, N_T)
        for i in range(2):
            out = d_out[i].cpu().numpy().view(np.uint64)
            inf = d_inf[i].cpu().numpy().astype(bool)
            for b in (0, 1, 2, 31, 64):
                assert pt(name, out[b], inf[b]) == oracle_c.msm_naive(name, srs[:ns[i]], limbs(rows[i][b])), (i, b)
    finally:
        ctx.close()


def _child(path):
    assert os.environ.get("KZGX_FIXED_JOINT_GLV") == "0"
    arrays = {}
    for name, C in CURVES:
        for key, (out, inf) in run_cases(name, C).items():
            arrays["%s:%s:out" % (name, key)] = out
            arrays["%s:%s:inf" % (name, key)] = inf
    np.savez(path, **arrays)


if __name__ == "__main__":
    _child(sys.argv[1])
