"""align_multi without a GPU: the C ABI declares and exports both calls, the ctypes binding matches the header, and the gang kernel
(lm_gang_kernel) meets the rules the LM cost kernel is held to -- three workgroups per CU, <= 168 VGPRs, no scratch in the main loop."""
import ctypes as C
import importlib.util
import os
import re
import subprocess

from tests import util

NAMES = ("fvh_vgicp_align_multi", "fvh_ndt_align_multi")


def _header():
    from fast_gicp_amd import build
    return re.sub(r"/\*.*?\*/", "", open(build.HEADER).read(), flags=re.S)


def test_both_calls_are_declared_and_exported():
    from fast_gicp_amd import build, capi
    declared = capi.declared_symbols()
    lib = build.build_lib()
    have = set(l.split()[-1] for l in subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True).stdout.splitlines())
    for n in NAMES:
        assert n in declared and n in have, n


def test_ctypes_argtypes_match_the_header():
    from fast_gicp_amd import capi
    hdr = _header()
    want = {"int": C.c_int}
    for n in NAMES:
        m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % n, hdr)
        assert m, n
        params = [p.strip() for p in m.group(1).split(",")]
        assert len(params) == len(capi.ALIGN_MULTI_ARGTYPES) == 6, params
        for p, t in zip(params, capi.ALIGN_MULTI_ARGTYPES):
            expect = C.c_void_p if "*" in p else want[p.split()[0]]
            assert t is expect, (n, p, t)
    assert re.search(r"1 <= k <= %d" % capi.MAX_MULTI, open(os.path.join(util.ROOT, "include", "fast_vgicp_hip.h")).read())


def _resources():
    spec = importlib.util.spec_from_file_location("kernel_resources", os.path.join(util.ROOT, "tools", "kernel_resources.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.kernel_resources()


def test_gang_kernel_stays_on_the_right_side_of_the_register_cliff():
    res = _resources()
    gang = {k: v for k, v in res.items() if "lm_gang_kernel<" in k}
    # every combination launch_cost can dispatch: {double, float} x {VGICP, NDT P2D, NDT D2D} x {per-transition, persistent} x {4, 1} x {LM, GN}
    assert len(gang) == 48, sorted(gang)
    assert not [k for k in gang if "cost_kernel" in k]  # (the existing instantiation counts must not see it)
    for k, v in gang.items():
        assert v["occupancy"] >= 3 and v["vgprs"] <= 168, (k, v)
        if ", true>(fvh::CostParams, fvh::GangParams)" in k:  # Gauss-Newton: co-resident like the others; its once-per-trip step may spill
            continue
        assert v["lds"] <= (32 * 1024 if ", true, " in k else 8 * 1024), (k, v)
        if ", true, " in k:
            assert v["vgpr_spill"] <= 32 and v["scratch"] <= 96, (k, v)
        else:
            assert v["vgpr_spill"] == 0 and v["scratch"] == 0, (k, v)


def test_gang_kernels_main_loop_has_no_scratch_access(tmp_path):
    from fast_gicp_amd import build as B
    out = tmp_path / "fvh.s"
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-mllvm", "-disable-machine-licm", "--cuda-device-only", "-S", "-DFVH_ASM_MARKS",
                           "-o", str(out), B.SOURCES[0]], stderr=subprocess.DEVNULL)
    text = out.read_text()
    for real in "df":
        for ch in "41":
            for mode in "012":
                name = "_ZN3fvh14lm_gang_kernelI%sLi%sELb1ELi%sELb0EEEvNS_10CostParamsENS_10GangParamsE" % (real, mode, ch)
                i = text.index(name + ":")
                body = text[i:text.index(".Lfunc_end", i)].split("\n")
                sec, scratch = "pre", {}
                for line in body:
                    line = line.strip()
                    m = re.match(r"; FVH_MARK (\d+)", line)
                    if m:
                        sec = int(m.group(1))
                    elif line.startswith("scratch_"):
                        scratch[sec] = scratch.get(sec, 0) + 1
                assert sec != "pre", name  # the marks are there
                main_loop = {k: v for k, v in scratch.items() if k != "pre" and k not in (7, 20, 21)}
                assert not main_loop, (name, scratch)
                assert sum(scratch.values()) <= 24, (name, scratch)


def test_cpp_classes_with_align_multi_compile(tmp_path):
    """alignMulti / alignBest on every class whose device LM goes through fvh_vgicp_align / fvh_ndt_align compile against the real headers"""
    src = tmp_path / "multi.cpp"
    src.write_text('''#include "fast_gicp_amd/registration.hpp"
using P = fast_gicp::PointXYZ;
int use(fast_gicp::FastVGICPCuda<P, P>& a, fast_gicp::NDTCuda<P, P>& n, fast_gicp::FastVGICP<P, P>& v, fast_gicp::PointCloud<P>& out) {
  const std::vector<fast_gicp::Matrix4f> g{fast_gicp::Matrix4f::Identity(), fast_gicp::Matrix4f::Identity()};
  const std::vector<fast_gicp::MultiAlignResult> r = a.alignMulti(g);
  const fast_gicp::MultiAlignResult& m = r[0];
  return (int)r.size() + (int)m.converged + m.nr_iterations + (int)(m.T(0, 3) + m.H[0] + m.final_error) + n.alignBest(g, 1.0, out) + v.alignBest(g, 1.0, out) +
         (int)n.alignMulti(g).size() + (int)v.alignMulti(g).size() + a.getMultiGridBlocks();
}
''')
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsyntax-only", "-I", os.path.join(util.ROOT, "include"), str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
