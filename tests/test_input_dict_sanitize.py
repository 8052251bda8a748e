"""The dictionary packer (csrc/host/dictpack.cpp) under AddressSanitizer and
UndefinedBehaviorSanitizer: a stand-alone program (csrc/host/
dictpack_stress.cpp) codes seeded random splits with several threads into
buffers of exactly the planned size and checks them with a byte-at-a-time
decoder.  No Python process loads sanitized code."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dict_packer_under_sanitizers(tmp_path):
    cxx = shutil.which("g++")  # the compiler libmrhost.so itself is built with (_build.build_cxx)
    assert cxx is not None, "g++ not found"
    exe = str(tmp_path / "dictpack_stress")
    src = [os.path.join(ROOT, "csrc", "host", "dictpack.cpp"), os.path.join(ROOT, "csrc", "host", "dictpack_stress.cpp")]
    r = subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-fno-sanitize-recover=all", "-o", exe] + src,
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1")
    r = subprocess.run([exe, "6", "2"], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert "dictpack_stress ok" in r.stdout
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
