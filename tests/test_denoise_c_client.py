"""The denoiser's entry points from a C caller: tests/helpers/c_denoise_client.c (C99, -pedantic, include/zdr.h) compiles and links
against libzdr_hip.so, and every call it makes with arguments the library must refuse is refused with ZDR_E_INVALID — before any HIP
call, so no GPU is needed."""
import os
import subprocess

from conftest import ROOT
from zdr_amd import _native

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def build_client(tmp_path):
    _native.lib()                                               # builds libzdr_hip.so if it is stale
    libdir = os.path.dirname(_native.LIB_PATH)
    exe = str(tmp_path / "c_denoise_client")
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{ROOT}/include",
                    os.path.join(ROOT, "tests", "helpers", "c_denoise_client.c"), "-o", exe, f"-L{libdir}", "-lzdr_hip", f"-L{ROCM}/lib", "-lamdhip64",
                    f"-Wl,-rpath,{libdir}", f"-Wl,-rpath,{ROCM}/lib"], check=True, capture_output=True, text=True)
    return exe


def test_a_c_caller_sees_the_denoiser_and_its_argument_checks(tmp_path):
    exe = build_client(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 1 and "usage" in r.stderr
    r = subprocess.run([exe, "--check"], capture_output=True, text=True, timeout=60)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and "UNEXPECTED" not in r.stdout
    assert r.stdout.count("as expected") == 6
