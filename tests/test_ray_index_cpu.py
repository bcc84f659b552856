"""csrc/sn_ray_index.h on the host: the ray index of a wave's 32 points (one multiplication per wave, one carry per lane) equals p / S.
The header is what the fp32 inference kernel compiles; tests/ray_index_check.cpp includes it, has its own main and needs no GPU."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_compiler():
    for cxx in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if cxx and shutil.which(cxx):
            return [shutil.which(cxx)]
    hipcc = shutil.which(os.environ.get("HIPCC", "hipcc"))
    assert hipcc, "no host C++ compiler found (c++, g++, clang++, hipcc)"
    return [hipcc, "-x", "c++"]


def test_ray_index_formula_equals_the_division(tmp_path):
    exe = str(tmp_path / "ray_index_check")
    src = os.path.join(REPO, "tests", "ray_index_check.cpp")
    base = _host_compiler() + ["-std=c++17", "-O1", "-g", src, "-o", exe]
    # with the undefined-behaviour sanitizer where the toolchain has its runtime (shifts and conversions of the 128-bit product)
    if subprocess.run(base + ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"], cwd=REPO, capture_output=True).returncode != 0:
        subprocess.run(base, check=True, cwd=REPO)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "comparisons equal p / S" in r.stdout, r.stdout
    assert int(r.stdout.split()[2]) > 1_000_000
