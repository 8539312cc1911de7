"""Builds tests/cpp/actor_boot_test.cpp (g++, C++17) and runs it: the C++ host methods of V(terminal observation) on time-limit rows
(ActorBoot / RolloutFusedValueBoot / RolloutFusedBoxBoot).  Once against tests/cpp/abi_stub.c plus a stub of the three new calls
(tests/cpp/actor_boot_stub.c), as a stand-alone program under AddressSanitizer and UBSan; once against libgymnet_amd.so, where the three
calls refuse a null handle (no GPU needed).  Fails without the feature: the methods and the exports do not exist."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
SRC = os.path.join(CPP, "actor_boot_test.cpp")
OUT_DIR = os.path.join(CPP, "build")
EXE = os.path.join(OUT_DIR, "actor_boot_test")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
INC = os.path.join(ROOT, "include")


def _build(gymnet):
    lib_dir = os.path.dirname(gymnet.LIB_PATH)
    os.makedirs(OUT_DIR, exist_ok=True)
    deps = [SRC, os.path.join(INC, "gymnet_amd.hpp"), os.path.join(INC, "gymnet_amd.h"), gymnet.LIB_PATH]
    if os.path.exists(EXE) and all(os.path.getmtime(EXE) >= os.path.getmtime(d) for d in deps):
        return EXE
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-D__HIP_PLATFORM_AMD__", "-I", INC,
           "-I", os.path.join(ROCM, "include"), SRC, "-o", EXE, "-L", lib_dir, "-lgymnet_amd", "-L", os.path.join(ROCM, "lib"), "-lamdhip64",
           f"-Wl,-rpath,{lib_dir}", f"-Wl,-rpath,{os.path.join(ROCM, 'lib')}"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return EXE


def test_cpp_mirror_against_the_stub_under_asan_and_ubsan(tmp_path):
    san = ["-O1", "-g", "-fno-omit-frame-pointer", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-I", INC]
    objs = []
    for name in ("abi_stub.c", "actor_boot_stub.c"):
        obj = str(tmp_path / (name[:-2] + ".o"))
        r = subprocess.run(["gcc", "-std=gnu11"] + san + ["-c", os.path.join(CPP, name), "-o", obj], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        objs.append(obj)
    exe = str(tmp_path / "actor_boot_stub_san")
    # the sanitizer runtime is linked statically: the program runs in the inherited environment, whatever that preloads
    r = subprocess.run(["g++", "-std=c++17", "-DBOOT_STUB", "-static-libasan"] + san + [SRC] + objs + ["-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1:detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([exe, "--stub"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0 and "stub: 0 failed" in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_cpp_actor_boot_cpu(gymnet):
    exe = _build(gymnet)
    r = subprocess.run([exe, "--cpu"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "cpu: 0 failed" in r.stdout
