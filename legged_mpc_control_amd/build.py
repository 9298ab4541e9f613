"""In-tree build of the HIP library (hipcc, gfx950 only) and the C++ host mirror test."""
from __future__ import annotations

import glob
import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
LIB = os.path.join(LIBDIR, "liblmpc.so")
ARCH = "gfx950"
# MFMA accumulators in the VGPR file (gfx950's register file is unified): without it the compiler parks the
# fp64 MFMA results in AGPRs and moves every element the VALU touches with v_accvgpr_read/write.  Measured:
# config 2 0.342 -> 0.329 ms, config 4 22.4 -> 22.0 ms (profiles/r02/diag_ab_configs.log).
HIP_FLAGS = ["-mllvm", "-amdgpu-mfma-vgpr-form"]
# Per-file machine scheduler (round 3, tools/ab_bench.sh / tools/hoqp_ab.sh, alternating runs, bit-identical
# results): the kernels are lone-wave, issue-in-order chains, and the ILP-oriented strategies interleave their
# independent work better than the default occupancy-oriented one -- max-ilp: config 2 0.2254-0.2284 ->
# 0.2198-0.2212 ms, config 4 19.61 -> 19.07-19.18 ms; iterative-ilp: the dual active set (config 2 --dense gi)
# 0.469 -> 0.459-0.461 ms, the WBC hierarchies 4.89 -> 4.78 ms.  (iterative-ilp crashes the compiler on
# lmpc_prep.hip, which keeps the default.)
# Floating-point contract of the dense path and the LDS Riccati kernel (the dense body is compiled into both
# lmpc_dense.hip and lmpc_lq.hip):
#   -ffp-contract=on: a * b + c becomes an fma only within one source expression (HIP's default contracts across
#     statements in the backend, where the result depends on how the surrounding code happens to split into basic
#     blocks).  A QP's bits must not depend on the kernel instance or launch that solves it (one- or two-wave
#     Riccati instance, the fused dense + Riccati launch); round 5 found the default broke that identity once the
#     kernel bodies became shared device functions.  0.6-1.4 % faster on configs 2-5 (tools/ab_bench.sh).
#   -fno-signed-zeros: lets the compiler drop additions of and multiplications into structural zeros of the unrolled
#     lane patterns (x + 0.0 = x up to the sign of a zero result; nothing here reads a zero's sign, and NaNs still
#     propagate to the NaN guard): config 4 9.74 -> 9.48 ms, config 5 3.33 -> 3.28 ms, config 2 within noise, every
#     GPU test at its tolerance (profiles/r05/fused/ab_math_flags.log; -freciprocal-math gained < 1 %, not adopted).
KERNEL_FP = ["-ffp-contract=on", "-fno-signed-zeros"]
SCHED_FLAGS = {
    "lmpc_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
    "lmpc_dense.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"] + KERNEL_FP,
    # the LDS Riccati kernel re-measured in round 5 (profiles/r05/fused/ab_sched.log): iterative-ilp config 4
    # 9.46 -> 9.26 ms, config 5 3.29 -> 3.12 ms; the dense body prefers max-ilp (config 2 +1.2 % under iterative-ilp),
    # so the fused dense + Riccati kernel has a file of its own
    "lmpc_lq.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"] + KERNEL_FP,
    "lmpc_fused.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"] + KERNEL_FP,
    "lmpc_gi.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"],
    "lmpc_hoqp.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"],
    # the fused controller + plant kernel: no FP flag, as lmpc_sim.hip and lmpc_lowlevel.hip (its results are theirs bit
    # for bit).  Without machine LICM the constants of the controller's sin / cos / atan2 / acos polynomials and the
    # stores' addresses are not hoisted out of the tick loop, where they stayed live through the plant step, which has
    # no register to spare: 66 VGPRs spilled (268 bytes of scratch) -> none (profiles/lowsim/registers.txt)
    "lmpc_lowsim.hip": ["-mllvm", "-disable-machine-licm"],
}

SOURCES = ["lmpc_kernels.hip", "lmpc_lq.hip", "lmpc_fused.hip", "lmpc_dense.hip", "lmpc_gi.hip", "lmpc_prep.hip", "lmpc_rollout.hip", "lmpc_hoqp.hip", "lmpc_wbc.hip", "lmpc_rbd.hip", "lmpc_sim.hip", "lmpc_contact.hip", "lmpc_stack.hip", "lmpc_est.hip", "lmpc_lowlevel.hip", "lmpc_lowsim.hip", "lmpc_capi.cpp",
           "hoqp_capi.cpp", "lmpc_host.cpp", "ConvexQPSolver.cpp"]


def _headers() -> list:
    """Every header a source of the library may include: csrc/*.h and the public include/lmpc/*, listed from the
    directories, so that a new header cannot be forgotten and leave a stale library behind."""
    return sorted(glob.glob(os.path.join(CSRC, "*.h"))) + sorted(glob.glob(os.path.join(ROOT, "include", "lmpc", "*")))


def _library_deps() -> list:
    return [os.path.join(CSRC, s) for s in SOURCES] + _headers()


def hipcc() -> str:
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _compile_cmd(source: str, output, defines=(), flags=()) -> list:
    """The compile line of one of SOURCES: the product's flags (HIP_FLAGS + that file's SCHED_FLAGS) + `flags`,
    -D`defines`; `output`: what says what to produce (["-c", "-o", obj])."""
    return [hipcc(), f"--offload-arch={ARCH}", "-O3", "-fPIC", "-std=c++17", "-Wno-unused-result",
            "-I", os.path.join(ROOT, "include"), "-I", CSRC] + list(output) + HIP_FLAGS + \
        SCHED_FLAGS.get(source, []) + list(flags) + [f"-D{d}" for d in defines] + [os.path.join(CSRC, source)]


def _compile_lib(out: str, objdir: str, defines=(), flags=(), verbose: bool = False, only=None) -> str:
    """liblmpc from SOURCES: one compile per source (HIP_FLAGS + that file's SCHED_FLAGS + `flags`, -D`defines`),
    run in parallel, then one link; written to `out` atomically.  `only`: compile just these sources and link the
    product's objects (lib/obj, built first) for the rest."""
    os.makedirs(objdir, exist_ok=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    procs, objs = [], []
    for s in SOURCES:
        if only is not None and s not in only:
            objs.append(os.path.join(LIBDIR, "obj", s + ".o"))
            continue
        obj = os.path.join(objdir, s + ".o")
        cmd = _compile_cmd(s, ["-c", "-o", obj], defines, flags)
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
        objs.append(obj)
    for cmd, pr in procs:
        if pr.wait() != 0:
            raise subprocess.CalledProcessError(pr.returncode, cmd)
    tmp = out + ".tmp"
    subprocess.run([hipcc(), f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", tmp] + objs, check=True)
    os.replace(tmp, out)
    return out


def device_metadata(source: str) -> dict:
    """{kernel name: {vgpr_count, sgpr_count, private_segment_fixed_size, vgpr_spill_count, sgpr_spill_count}} of one of
    SOURCES, compiled for the device alone with the product's compile line (_compile_cmd) and read from the code object's
    metadata in the assembly.  For tests that hold a kernel to "no scratch": a compiler upgrade can bring spills back without changing
    a result."""
    import re

    asm = os.path.join(LIBDIR, "build", source + ".s")  # kept: compiled again only when a source or header is newer
    if _stale(asm, [os.path.join(CSRC, source), os.path.abspath(__file__)] + _headers()):
        os.makedirs(os.path.dirname(asm), exist_ok=True)
        subprocess.run(_compile_cmd(source, ["--cuda-device-only", "-S", "-o", asm + ".tmp"],
                                    flags=["-Wno-unused-command-line-argument"]), check=True)
        os.replace(asm + ".tmp", asm)
    text = open(asm).read()
    out, cur = {}, {}
    for line in text.splitlines():
        m = re.match(r"\s+\.(name|vgpr_count|sgpr_count|private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count):\s+(\S+)$",
                     line)
        if m and m.group(1) == "name":
            cur["name"] = m.group(2)
        elif m:
            cur[m.group(1)] = int(m.group(2))
        if line.strip().startswith(".wavefront_size") and "name" in cur:
            out[cur.pop("name")] = cur
            cur = {}
    return out


def build_native(force: bool = False, verbose: bool = False) -> str:
    if not force and not _stale(LIB, _library_deps() + [os.path.abspath(__file__)]):
        return LIB
    return _compile_lib(LIB, os.path.join(LIBDIR, "obj"), verbose=verbose)


MULTI_LIB = os.path.join(LIBDIR, "liblmpc_multi.so")


def build_multi(force: bool = False, verbose: bool = False) -> str:
    """liblmpc_multi.so (include/lmpc/lmpc_multi.h): several devices from one process, RCCL for the batch
    scatter / gather.  Links liblmpc.so (found next to it at run time) and librccl."""
    src = os.path.join(CSRC, "lmpc_multi.cpp")
    deps = [src, LIB, os.path.join(ROOT, "include", "lmpc", "lmpc_multi.h"), os.path.join(ROOT, "include", "lmpc", "lmpc.h"),
            os.path.abspath(__file__)]
    if not force and not _stale(MULTI_LIB, deps):
        return MULTI_LIB
    tmp = MULTI_LIB + ".tmp"
    cmd = [hipcc(), f"--offload-arch={ARCH}", "-O2", "-fPIC", "-shared", "-std=c++17", "-I", os.path.join(ROOT, "include"), "-o", tmp, src,
           "-L", LIBDIR, "-llmpc", "-Wl,-rpath,$ORIGIN", "-L/opt/rocm/lib", "-lrccl", "-Wl,-rpath,/opt/rocm/lib"]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    os.replace(tmp, MULTI_LIB)
    return MULTI_LIB


def build_stamps(force: bool = False) -> str:
    """Diagnostic library with in-kernel phase cycle stamps (tools/stamps_probe.py); never shipped as the product."""
    return build_variant("stamps", ["LMPC_STAMPS"], force)


def build_variant(tag: str, defines, force: bool = False, flags=()) -> str:
    """Diagnostic library variant (extra -D flags, extra compiler flags) under tools/build/; never shipped as the
    product."""
    out = os.path.join(ROOT, "tools", "build", f"liblmpc_{tag}.so")
    if not force and not _stale(out, _library_deps()):
        return out
    return _compile_lib(out, os.path.join(ROOT, "tools", "build", f"obj_{tag}"), defines=defines, flags=flags)


TEST_BUILD = os.path.join(ROOT, "tests", "build")
# Test-only library variants (tests/test_gpu_kkt.py), never the product: bugs re-injected into the LDS Riccati
# kernel's forward sweep -- round 4's lost "+ za", and the next stage's yaw read for A_k -- with the polish's KKT
# certificate (the product's verification) and without it (LMPC_KKT_OFF: round 4's verification).
TEST_VARIANTS = {
    "bugza": (["LMPC_BUG_ZA"], ("lmpc_lq.hip", "lmpc_fused.hip")),
    "bugza_nokkt": (["LMPC_BUG_ZA", "LMPC_KKT_OFF"], ("lmpc_lq.hip", "lmpc_fused.hip")),
    "bugyaw": (["LMPC_BUG_YAW"], ("lmpc_lq.hip", "lmpc_fused.hip")),
    "bugyaw_nokkt": (["LMPC_BUG_YAW", "LMPC_KKT_OFF"], ("lmpc_lq.hip", "lmpc_fused.hip")),
    # the dense polish with every round refactorised (no range-space updates): tests/test_gpu_kkt.py checks that the
    # product's updates reach the same iteration words and forces
    "noschur": (["LMPC_POLISH_SCHUR=0"], ("lmpc_dense.hip", "lmpc_lq.hip", "lmpc_fused.hip")),
    # the range-space rounds' per-QP counters (rounds, entries, columns, largest size, longest run) and the check of
    # leg_free against the bases: tests/test_gpu_schur_rounds.py shows with them that its batches reach the code
    "schurdiag": (["LMPC_SCHUR_DIAG"], ("lmpc_dense.hip", "lmpc_lq.hip", "lmpc_fused.hip")),
    # the dense path's diagonal tiles by diag_inverse (T and W = L^-1 in tiles of their own, two MFMAs per pivot) in
    # place of diag_inverse_merged: tests/test_gpu_dense_diag.py checks that the merged tile leaves every bit of the
    # answers where it was
    "diag2tile": (["LMPC_DIAG_TWO_TILES"], ("lmpc_dense.hip", "lmpc_lq.hip", "lmpc_fused.hip")),
    # the dense polish with leg_basis called where a round needs a basis, in place of the per-QP face-set table:
    # tests/test_gpu_basis_table.py checks that the table leaves every bit of the answers where it was
    "basisdirect": (["LMPC_BASIS_TABLE=0"], ("lmpc_dense.hip", "lmpc_lq.hip", "lmpc_fused.hip")),
    # the product plus lmpc_debug_basis_probe: the table's builder and reader against leg_basis on all 32 face words
    "basisprobe": (["LMPC_BASIS_PROBE"], ("lmpc_dense.hip",)),
}


def build_test_variants(force: bool = False) -> dict:
    """The TEST_VARIANTS libraries under tests/build/ (only the named sources recompiled; the rest are the product's
    objects, so build_native() first)."""
    build_native()
    out = {}
    for tag, (defines, only) in TEST_VARIANTS.items():
        path = os.path.join(TEST_BUILD, f"liblmpc_{tag}.so")
        if force or _stale(path, _library_deps() + [LIB]):
            _compile_lib(path, os.path.join(TEST_BUILD, f"obj_{tag}"), defines=defines, only=only)
        out[tag] = path
    return out


def _build_program(src: str, out: str, force: bool, deps=(), flags=(), includes=(), libs=("-llmpc",)) -> str:
    """A C++ program over liblmpc.so (found at run time where it was built); `deps`: what else it is made from,
    `includes`: directories searched before include/, `libs`: what it links from lib/."""
    if not force and not _stale(out, [src, LIB] + list(deps)):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [hipcc(), "-O2", "-std=c++17"] + list(flags) + [a for i in includes for a in ("-I", i)] + \
        ["-I", os.path.join(ROOT, "include"), "-o", out, src, "-L", LIBDIR] + list(libs) + [f"-Wl,-rpath,{LIBDIR}"]
    subprocess.run(cmd, check=True)
    return out


def _cpp_test(name: str, force: bool, **kw) -> str:
    return _build_program(os.path.join(ROOT, "tests", "cpp", f"{name}.cpp"),
                          os.path.join(ROOT, "tests", "cpp", "build", name), force, **kw)


def build_cpp_test(force: bool = False) -> str:
    """C++ program that drives legged::ConvexQPSolver exactly like ConvexMpc::grf_update."""
    return _cpp_test("grf_update_test", force)


def build_cpp_multi_test(force: bool = False) -> str:
    """C++ host over the multi-device C-ABI (tests/cpp/multi_test.cpp): shards a batch without PyTorch."""
    return _cpp_test("multi_test", force, deps=[MULTI_LIB], libs=("-llmpc_multi", "-llmpc"))


def build_cpp_eigen_test(force: bool = False) -> str:
    """The reference's ConvexMpc lines over include/lmpc/ConvexQPSolverEigen.hpp (tests/cpp/eigen_dropin_test.cpp),
    compiled against the test stand-ins in tests/cpp/eigen_dropin/ (no Eigen / ROS in this image)."""
    return _cpp_test("eigen_dropin_test", force, deps=[os.path.join(ROOT, "include", "lmpc", "ConvexQPSolverEigen.hpp")],
                     flags=["-Wall"], includes=[os.path.join(ROOT, "tests", "cpp", "eigen_dropin")])


def build_cpp_hoqp_test(force: bool = False) -> str:
    """C++ program running the reference's HoQp test (ho_qp_test.cpp) against legged::HoQp (include/lmpc/HoQp.hpp)."""
    return _cpp_test("ho_qp_test", force, deps=[os.path.join(ROOT, "include", "lmpc", "HoQp.hpp")])


def build_tool_cpp(name: str, force: bool = False) -> str:
    """Dev tool program over liblmpc.so (tools/<name>.cpp -> tools/build/<name>); never shipped."""
    return _build_program(os.path.join(ROOT, "tools", f"{name}.cpp"), os.path.join(ROOT, "tools", "build", name), force)


def host_cxx() -> str:
    for c in (os.environ.get("CXX"), "g++", "c++", "clang++"):
        path = shutil.which(c) if c else None
        if path:
            return path
    raise RuntimeError("no host C++ compiler found")


def _build_host_check(name: str, csrc_headers, public_headers, force: bool) -> str:
    """tests/cpp/<name>.cpp, a stand-alone program over the named csrc/ and include/lmpc/ headers, built by the host
    compiler with AddressSanitizer and UBSan: host code only, no HIP and no liblmpc.so."""
    src = os.path.join(ROOT, "tests", "cpp", f"{name}.cpp")
    out = os.path.join(ROOT, "tests", "cpp", "build", name)
    deps = [src] + [os.path.join(CSRC, h) for h in csrc_headers] + \
        [os.path.join(ROOT, "include", "lmpc", h) for h in public_headers]
    if not force and not _stale(out, deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    cmd = [host_cxx(), "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", out, src]
    subprocess.run(cmd, check=True)
    return out


def build_cpp_sim_check(force: bool = False) -> str:
    """The plant step of csrc/lmpc_sim_common.h on a few robots (tests/cpp/sim_host_check.cpp)."""
    return _build_host_check("sim_host_check", ("lmpc_sim_common.h", "lmpc_rbd_common.h"), ("lmpc_sim.h", "lmpc_rbd.h"), force)


def build_cpp_contact_check(force: bool = False) -> str:
    """The contact model of csrc/lmpc_contact_common.h (tests/cpp/contact_host_check.cpp)."""
    return _build_host_check("contact_host_check", ("lmpc_contact_common.h", "lmpc_sim_common.h", "lmpc_rbd_common.h"),
                             ("lmpc_contact.h", "lmpc_sim.h", "lmpc_rbd.h"), force)


def build_cpp_est_check(force: bool = False) -> str:
    """The estimator of csrc/lmpc_est_common.h (tests/cpp/est_host_check.cpp)."""
    return _build_host_check("est_host_check", ("lmpc_est_common.h", "lmpc_rbd_common.h", "lmpc_common.h"),
                             ("lmpc_est.h", "lmpc_sim.h", "lmpc_rbd.h"), force)


def build_cpp_lowlevel_check(force: bool = False) -> str:
    """The joint-PD controller of csrc/lmpc_lowlevel_common.h (tests/cpp/lowlevel_host_check.cpp)."""
    return _build_host_check("lowlevel_host_check", ("lmpc_lowlevel_common.h", "lmpc_common.h"),
                             ("lmpc_lowlevel.h", "lmpc_sim.h", "lmpc_rbd.h", "lmpc.h"), force)


def build_cpp_lowsim_check(force: bool = False) -> str:
    """lmpc_lowsim_run's host function (csrc/lmpc_lowsim_common.h) against the explicit loop of controller and plant
    steps (tests/cpp/lowsim_host_check.cpp)."""
    return _build_host_check("lowsim_host_check", ("lmpc_lowlevel_common.h", "lmpc_sim_common.h", "lmpc_rbd_common.h",
                                                   "lmpc_common.h", "lmpc_lowsim_common.h"),
                             ("lmpc_lowsim.h", "lmpc_lowlevel.h", "lmpc_sim.h", "lmpc_rbd.h", "lmpc.h"), force)


def build_cpp_order_check(force: bool = False) -> str:
    """The cross-stream ordering and the grown buffer of csrc/lmpc_order.h over a logging stand-in for HIP
    (tests/cpp/order_host_check.cpp)."""
    return _build_host_check("order_host_check", ("lmpc_order.h",), ("lmpc.h",), force)


if __name__ == "__main__":
    print(build_native(force=True, verbose=True))
    print(build_multi(force=True, verbose=True))
