"""GPU tests through the host C++ classes / pygicp: the reference's own test (src/test/gicp_test.cpp:147-201) re-stated --
forward / backward / swap-and-set-source / swap-and-set-target for VGICP_CUDA and NDT_CUDA with default parameters,
tolerances 0.05 m / 1 deg / hasConverged -- plus equality of the host-LM and device-LM paths and of the neighbour methods."""
import numpy as np
import pytest

from tests import util

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pygicp():
    import pygicp
    return pygicp


@pytest.fixture(scope="module")
def data():
    t, s = util.bundled_pair(origin_filter=False, leaf=0.2, exact_voxelgrid=True)  # gicp_test.cpp:55-65
    return t.astype(np.float64), s.astype(np.float64), util.relative_pose()


def _check(gt, T, converged, label):
    te, re_ = util.pose_error(gt, np.asarray(T, np.float64))
    assert te < 0.05, (label, te)
    assert re_ < np.radians(1.0), (label, re_)
    assert converged, label


@pytest.mark.parametrize("method", ["VGICP_CUDA", "NDT_CUDA"])
def test_gicp_test_alignment(pygicp, data, method):
    target, source, gt = data
    create = (lambda: pygicp.FastVGICPCuda()) if method == "VGICP_CUDA" else (lambda: pygicp.NDTCuda())
    reg = create()
    reg.set_input_target(target); reg.set_input_source(source)
    _check(gt, reg.align(), reg.has_converged(), "FORWARD TEST")
    reg.set_input_target(source); reg.set_input_source(target)
    _check(gt, np.linalg.inv(reg.align().astype(np.float64)), reg.has_converged(), "BACKWARD TEST")
    reg = create()
    reg.set_input_source(target); reg.swap_source_and_target(); reg.set_input_source(source)
    _check(gt, reg.align(), reg.has_converged(), "SWAP AND SET SOURCE TEST")
    reg = create()
    reg.set_input_target(source); reg.swap_source_and_target(); reg.set_input_target(target)
    _check(gt, reg.align(), reg.has_converged(), "SWAP AND SET TARGET TEST")


@pytest.mark.parametrize("cls", ["FastVGICPCuda", "NDTCuda"])
def test_host_lm_equals_device_lm(pygicp, data, cls):
    """The reference's host loop (linearize / compute_error virtuals -> update_correspondences + compute_error) and the
    device-resident loop must agree to fp64 rounding."""
    target, source, _ = data
    out = []
    for dev in (True, False):
        reg = getattr(pygicp, cls)()
        reg.set_use_device_lm(dev)
        reg.set_input_target(target); reg.set_input_source(source)
        T = reg.align()
        out.append((T, reg.get_final_hessian(), reg.has_converged(), reg.get_fitness_score()))
    assert np.array_equal(out[0][0], out[1][0])  # float32 final_transformation_
    assert util.rel_err(out[0][1], out[1][1]) < 1e-10
    assert out[0][2] and out[1][2]
    assert out[0][3] == out[1][3]


@pytest.mark.parametrize("cls", ["FastVGICPCuda", "FastVGICP", "FastGICP", "NDTCuda"])
def test_gauss_newton_optimizer_matches_oracle(pygicp, data, cls):
    """LSQ_OPTIMIZER_TYPE::GaussNewton (lsq_registration_impl.hpp:94-121) through the host classes, against the oracle's step_gn at 1e-4
    (north_star), Hessian included. Since round 5 the Gauss-Newton loop is device-resident like Levenberg-Marquardt (fvh_lm_params::optimizer:
    one linearisation per transition inside the kernel, the step always taken); the reference's host loop on the device's linearize()
    (set_use_device_lm(False)) must give the same registration to fp64 rounding."""
    from oracle import oracle as O
    target, source, gt = data
    reg = getattr(pygicp, cls)()
    reg.set_lsq_type("GN")
    reg.set_input_target(target); reg.set_input_source(source)
    T = reg.align()
    host = getattr(pygicp, cls)()
    host.set_lsq_type("GN"); host.set_use_device_lm(False)
    host.set_input_target(target); host.set_input_source(source)
    Th = host.align()
    assert np.array_equal(T, Th) and reg.has_converged() and host.has_converged()  # float32 final_transformation_
    assert util.rel_err(reg.get_final_hessian(), host.get_final_hessian()) < 1e-10
    if cls == "NDTCuda":
        g = O.NDT()
    else:
        g = O.FastVGICP(search=O.DIRECT1)
        if cls == "FastGICP":
            g.set_gicp_mode(True)
    g.set_optimizer("GN")
    g.set_target(target.astype(np.float32)); g.set_source(source.astype(np.float32))
    ro = g.align()
    assert reg.has_converged() and ro["converged"] and ro["num_error_evals"] == 0
    assert util.rel_err(T, ro["T"].astype(np.float32)) < 1e-4
    assert util.rel_err(reg.get_final_hessian(), ro["H"]) < 1e-4
    _check(gt, T, True, cls + " Gauss-Newton")
    with pytest.raises(Exception):
        reg.set_lsq_type("Newton")


def test_neighbor_methods_agree(pygicp, data):
    """CPU_PARALLEL_KDTREE -- the reference's default -- asks for exact k-NN lists: served by the device search by default (round 6), by the host
    kd-tree of include/fast_gicp_amd/kdtree.hpp after set_host_kdtree(True); GPU_BRUTEFORCE is the device search. The same neighbours ->
    the same covariances -> bit-identical registrations, all three ways."""
    target, source, _ = data
    res = []
    for m, host in (("CPU_PARALLEL_KDTREE", False), ("CPU_PARALLEL_KDTREE", True), ("GPU_BRUTEFORCE", False)):
        reg = pygicp.FastVGICPCuda()
        reg.set_nearest_neighbor_search_method(m)
        if host:
            reg.set_host_kdtree(True)
        reg.set_input_target(target); reg.set_input_source(source)
        res.append(reg.align())
    assert np.array_equal(res[0], res[1]) and np.array_equal(res[0], res[2])
    # the host tree itself (built by OpenMP tasks) against the device lists, row by row
    from fast_gicp_amd import capi
    c = capi.VGICPCore(0)
    c.set_target_cloud(target.astype(np.float32)); c.find_target_neighbors(20)
    dev = c.get_neighbors("target")
    assert np.array_equal(np.asarray(pygicp._kdtree_knn(target, 20)), dev)
    c.close()


def test_align_points_and_evaluate_cost(pygicp, data):
    target, source, gt = data
    for method in ("VGICP_CUDA", "NDT_CUDA"):
        T = pygicp.align_points(target, source, method=method, neighbor_search_method="DIRECT7")
        te, re_ = util.pose_error(gt, T)
        assert te < 0.06 and re_ < np.radians(1.0)
    reg = pygicp.FastVGICPCuda()
    reg.set_input_target(target); reg.set_input_source(source)
    e, H, b = reg.evaluate_cost(np.eye(4))
    assert e > 0 and np.allclose(H, H.T) and np.all(np.linalg.eigvalsh(H) > 0) and b.shape == (6,)


def test_rbf_kernel_mode(pygicp, data):
    target, source, gt = data
    reg = pygicp.FastVGICPCuda()
    reg.set_nearest_neighbor_search_method("GPU_RBF_KERNEL")
    reg.set_kernel_width(0.5)
    reg.set_input_target(target); reg.set_input_source(source)
    _check(gt, reg.align(), reg.has_converged(), "RBF")


def test_fast_gicp_covariance_accessors(pygicp, data):
    """gicp/fast_gicp.hpp:60-70: get*Covariances returns what setInput* estimated (k-NN + PLANE: eigenvalues 1e-3, 1, 1);
    set*Covariances replaces them -- feeding the read-back values gives the same alignment, isotropic ones a different one."""
    target, source, gt = data
    reg = pygicp.FastGICP()
    reg.set_input_target(target); reg.set_input_source(source)
    T0 = reg.align()
    cs, ct = reg.get_source_covariances(), reg.get_target_covariances()
    assert cs.shape == (len(source), 3, 3) and ct.shape == (len(target), 3, 3)
    assert np.allclose(cs, np.swapaxes(cs, 1, 2))
    w = np.linalg.eigvalsh(cs[::97])
    assert np.allclose(w, [1e-3, 1.0, 1.0], atol=1e-4)
    reg2 = pygicp.FastGICP()
    reg2.set_input_target(target); reg2.set_input_source(source)
    reg2.set_source_covariances(cs); reg2.set_target_covariances(ct)
    T1 = reg2.align()
    assert util.rel_err(T1, T0) < 1e-6
    reg2.set_source_covariances(np.tile(np.eye(3), (len(source), 1, 1))); reg2.set_target_covariances(np.tile(np.eye(3), (len(target), 1, 1)))
    T2 = reg2.align()  # plain point-to-point ICP weights: a different (and on this pair slightly worse, ~6 cm) optimum
    te, re_ = util.pose_error(gt, np.asarray(T2, np.float64))
    assert reg2.has_converged() and te < 0.15 and re_ < np.radians(2.0)
    assert util.rel_err(T2, T0) > 1e-6
    with pytest.raises(Exception):
        reg2.set_source_covariances(cs[:10])


def test_debug_print_table_from_the_device_lm(pygicp, data, capfd):
    """setDebugPrint(true): the reference prints one line per trial step (lsq_registration_impl.hpp:143-149). The device-resident
    LM records those rows on the GPU and the host prints the same table afterwards; it must equal, value for value, the table the
    host-driven loop prints while it runs, and the oracle's."""
    from oracle import oracle as O
    target, source, _ = data
    tables = {}
    for dev in (True, False):
        reg = pygicp.FastVGICPCuda()
        reg.set_nearest_neighbor_search_method("GPU_BRUTEFORCE")
        reg.set_use_device_lm(dev)
        reg.set_debug_print(True)
        reg.set_input_target(target); reg.set_input_source(source)
        capfd.readouterr()
        reg.align()
        import sys
        sys.stdout.flush()
        out = capfd.readouterr().out
        rows = [l.split() for l in out.splitlines() if l.strip() and l.split()[0].isdigit()]
        assert out.count("--- LM optimization ---") >= 3 and len(rows) >= 3
        tables[dev] = np.array([[float(v) for v in r[:6]] for r in rows])
        assert all((len(r) == 7 and r[6] == "x") == (float(r[3]) > 0) for r in rows)
    assert tables[True].shape == tables[False].shape
    np.testing.assert_allclose(tables[True], tables[False], rtol=1e-5, atol=1e-12)  # (%g prints 6 significant digits)


def test_lm_trace_rows_through_the_abi(data):
    from fast_gicp_amd import capi
    target, source, _ = data
    c = capi.VGICPCore(0)
    c.set_target_cloud(target); c.find_target_neighbors(20); c.calculate_target_covariances(); c.create_target_voxelmap()
    c.set_source_cloud(source); c.find_source_neighbors(20); c.calculate_source_covariances()
    r0 = c.align()
    assert len(c.get_lm_trace()) == 0          # off by default
    c.set_lm_trace(True)
    r = c.align()
    t = c.get_lm_trace()
    assert t.shape == (r["num_error_evals"], 6) and np.array_equal(r["T"], r0["T"])
    assert np.all(t[:, 3][t[:, 0] == 0] == t[:, 3][t[:, 0] == 0])
    assert t[-1, 1] <= t[0, 1] and np.all(t[:, 4] > 0) and np.all(t[:, 5] > 0)   # y0 decreases over the run; lambda, |d| positive
    assert np.all((t[:, 2] < t[:, 1]) == (t[:, 3] > 0))                            # rho > 0  <=>  the trial lowered the error (denominator > 0)
    c.close()


@pytest.mark.parametrize("k", [10, 15, 32])
def test_vgicp_honours_k_correspondences_like_the_cpu_class(pygicp, k):
    """main.cpp:102-108: align_points(method="VGICP") builds the CPU FastVGICP, whose setCorrespondenceRandomness(k) is real
    (k_correspondences defaults to 15 in align_points, main.cpp:155-167), while FastVGICPCuda's is empty (k stays 20,
    fast_vgicp_cuda_impl.hpp:38). Round 2 aliased "VGICP" to the CUDA class and ran k = 20 whatever the caller asked: here the
    result must equal the ORACLE's FastVGICP with the same k (1e-4, north_star), and differ from the k = 20 result."""
    from oracle import oracle as O
    tgt, src = util.bundled_pair()
    T = pygicp.align_points(tgt.astype(np.float64), src.astype(np.float64), method="VGICP", k_correspondences=k, voxel_resolution=1.0, neighbor_search_method="DIRECT7")
    g = O.FastVGICP(k=k, search=O.DIRECT7)
    g.set_target(tgt); g.set_source(src)
    ro = g.align()
    assert ro["converged"]
    assert util.rel_err(T, ro["T"].astype(np.float32)) < 1e-4, (k, util.rel_err(T, ro["T"]))
    T20 = pygicp.align_points(tgt.astype(np.float64), src.astype(np.float64), method="VGICP_CUDA", k_correspondences=k, voxel_resolution=1.0, neighbor_search_method="DIRECT7")
    g20 = O.FastVGICP(k=20, search=O.DIRECT7)
    g20.set_target(tgt); g20.set_source(src)
    assert util.rel_err(T20, g20.align()["T"].astype(np.float32)) < 1e-4  # the CUDA class: k = 20 whatever was asked, as in the reference
    assert not np.array_equal(T, T20)
    # the class itself (main.cpp:192-196 + the FastGICP methods it inherits there)
    reg = pygicp.FastVGICP()
    reg.set_num_threads(4); reg.set_correspondence_randomness(k); reg.set_max_correspondence_distance(1.0)
    reg.set_resolution(1.0); reg.set_neighbor_search_method("DIRECT7")
    reg.set_input_target(tgt.astype(np.float64)); reg.set_input_source(src.astype(np.float64))
    assert np.array_equal(reg.align(), T) and reg.has_converged()
    assert isinstance(reg, pygicp.FastGICP) and isinstance(reg, pygicp.LsqRegistration)  # main.cpp:192: FastVGICP derives from FastGICP


def test_vgicp_uses_target_covariances_and_resolution_set_after_the_target(pygicp):
    """fast_vgicp_impl.hpp:56-63,120-123: the CPU class builds its voxel map lazily, inside the first linearisation of an align, from the
    target covariances and the resolution that are current THEN -- so set_target_covariances() and set_resolution() called after
    set_input_target() take effect. The host class here builds the map eagerly: both setters must rebuild it (they did not,
    and user covariances were silently ignored). Checked against the oracle driven with the same covariances / resolution."""
    from oracle import oracle as O
    tgt, src = util.bundled_pair(leaf=0.25)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(len(tgt), 3, 3)) * 0.05
    cov_t = A @ np.swapaxes(A, 1, 2) + np.eye(3) * 1e-3  # arbitrary SPD covariances, nothing like the k-NN PLANE ones

    def oracle(res, covs):
        g = O.FastVGICP(k=20, search=O.DIRECT7, resolution=res)
        g.set_target(tgt); g.set_source(src)
        if covs is not None:
            g.set_target_covs(covs)
        r = g.align()
        assert r["converged"]
        return r["T"].astype(np.float32)

    def make(res):
        reg = pygicp.FastVGICP()
        reg.set_resolution(res); reg.set_neighbor_search_method("DIRECT7")
        reg.set_input_target(tgt.astype(np.float64)); reg.set_input_source(src.astype(np.float64))
        return reg

    reg = make(1.0)
    T_default = reg.align()
    assert util.rel_err(T_default, oracle(1.0, None)) < 1e-4
    reg.set_target_covariances(cov_t)  # AFTER the target (and its map) exist
    T_user = reg.align()
    assert reg.has_converged()
    assert util.rel_err(T_user, oracle(1.0, cov_t)) < 1e-4
    assert util.rel_err(T_user, T_default) > 1e-5  # (the user covariances do change the optimum: ignoring them cannot pass)
    reg = make(1.0)
    reg.set_resolution(2.0)  # AFTER the target
    T_res = reg.align()
    assert util.rel_err(T_res, oracle(2.0, None)) < 1e-4
    assert util.rel_err(T_res, T_default) > 1e-6


def test_pipelined_calls_of_the_class_equal_the_sequential_loop():
    """FastVGICPCuda.align_async / prepare_next_source / align_wait / adopt_prepared_source (not in the reference: the next scan's conversion, upload,
    sort, k-NN and covariances beside the running LM kernel) register what set_input_source + align register."""
    import pygicp
    from tests import util
    frames = [pygicp.downsample(util.lidar_frame(i).astype(np.float64), 0.25) for i in range(5)]

    def make():
        reg = pygicp.FastVGICPCuda()
        reg.set_resolution(1.0); reg.set_neighbor_search_method("DIRECT7")
        reg.set_input_target(frames[0])
        return reg

    reg = make()
    seq = []
    for i in range(1, 5):
        reg.set_input_source(frames[i])
        seq.append(reg.align().copy())
        reg.swap_source_and_target()
    reg = make()
    reg.prepare_next_source(frames[1]); reg.adopt_prepared_source()
    for i in range(1, 5):
        reg.align_async()
        if i + 1 < 5:
            reg.prepare_next_source(frames[i + 1])
        T = reg.align_wait()
        assert reg.has_converged()
        assert np.abs(T - seq[i - 1]).max() < 1e-6, i
        reg.swap_source_and_target()
        if i + 1 < 5:
            reg.adopt_prepared_source()


def test_pipelined_calls_of_ndt_equal_the_sequential_loop():
    """NDTCuda.align_async / prepare_next_source / align_wait / adopt_prepared_source on host clouds (not in the reference)."""
    import pygicp
    from tests import util
    frames = [pygicp.downsample(util.lidar_frame(i).astype(np.float64), 0.25) for i in range(5)]

    def make():
        reg = pygicp.NDTCuda()
        reg.set_resolution(1.0); reg.set_neighbor_search_method("DIRECT7"); reg.set_distance_mode("D2D")
        reg.set_input_target(frames[0])
        return reg

    reg = make()
    seq = []
    for i in range(1, 5):
        reg.set_input_source(frames[i])
        seq.append(reg.align().copy())
        reg.swap_source_and_target()
    reg = make()
    reg.prepare_next_source(frames[1])
    for i in range(1, 5):
        reg.adopt_prepared_source()
        reg.align_async()
        if i + 1 < 5:
            reg.prepare_next_source(frames[i + 1])
        T = reg.align_wait()
        assert reg.has_converged()
        assert np.abs(T - seq[i - 1]).max() < 1e-6, i
        reg.swap_source_and_target()


def test_class_errors_name_the_call_and_carry_the_handles_text(pygicp):
    """What the classes throw when the library refuses a call: "<label> failed (status N): <the handle's last_error text>", the label being the
    C call without its fvh_<handle>_ prefix (cloud setters: without _strided). Checked through the real library on the refusals a caller can
    reach without breaking anything; the text is compared with what the same misuse of a bare handle reports."""
    import re
    from fast_gicp_amd import capi
    rng = np.random.default_rng(11)
    cloud = rng.uniform(-2.0, 2.0, size=(64, 3))

    def library_text(handle, misuse):
        with pytest.raises(capi.FvhError) as e:
            misuse(handle)
        handle.close()
        return re.match(r"fvh_\w+: status \d+: (.*)$", str(e.value), re.S).group(1)

    def raised(label, call, text):
        with pytest.raises(RuntimeError) as e:
            call()
        msg = str(e.value)
        assert re.match(re.escape(label) + r" failed \(status \d+\): ", msg), msg
        assert text and msg.endswith("): " + text), (msg, text)

    raised("align_wait", pygicp.NDTCuda().align_wait, library_text(capi.NDTCore(0), lambda c: c.align_wait()))
    raised("align_wait", pygicp.FastVGICPCuda().align_wait, library_text(capi.VGICPCore(0), lambda c: c.align_wait()))

    def swap_an_incremental_target(c):
        c.map_begin()
        c.swap_source_and_target()
    reg = pygicp.FastVGICPCuda()
    reg.begin_incremental_target()
    reg.set_input_source(cloud)
    reg.insert_source_into_target(np.eye(4))
    raised("swap_source_and_target", reg.swap_source_and_target, library_text(capi.VGICPCore(0), swap_an_incremental_target))
    T = reg.align()  # the handle is as usable as before (the scan against the map made of it; accuracy is other tests' business)
    assert reg.has_converged() and np.isfinite(T).all()

    gicp = pygicp.FastGICP()
    gicp.set_input_target(cloud); gicp.set_input_source(cloud)
    with pytest.raises(ValueError, match="setSourceCovariances: one covariance per source point"):  # refused by the class, before the library
        gicp.set_source_covariances(np.tile(np.eye(3), (63, 1, 1)))
    gicp.set_source_covariances(np.tile(np.eye(3), (64, 1, 1)))
