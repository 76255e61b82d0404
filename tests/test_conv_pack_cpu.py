"""The host-side packers of a convolution's parameter block (csrc/conv_pack.cpp) on the CPU: tests/host/conv_pack_check.cpp, a program
of its own, built together with conv_pack.cpp under the address and undefined-behaviour sanitizers and run as an ordinary executable.
It walks every (class, row, k) of every weight copy -- position, the exact bf16x3 split, the fp16x2 split within the bound
test_h2_model_cpu.py asserts, zero padding and slack -- and every granule of the tap table; the sanitizers see every write."""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "accel_amd", "csrc")


def test_conv_pack_check_under_sanitizers(tmp_path):
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))      # conv_pack.cpp uses _Float16: the compiler the library is built with
    assert hipcc, "hipcc not found"
    exe = str(tmp_path / "conv_pack_check")
    # host code only: the sanitizers go to the host compilation (-Xarch_host), nothing here is compiled for or run on a GPU
    cmd = [hipcc, "-x", "c++", "-std=c++17", "-O1", "-g", "-Wall", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
           os.path.join(HERE, "host", "conv_pack_check.cpp"), os.path.join(CSRC, "conv_pack.cpp"), "-o", exe]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(run.stdout)
    assert run.returncode == 0 and run.stdout.strip().endswith("conv_pack: ok"), run.stdout[-4000:] + run.stderr[-4000:]
