"""Host-only check of csrc/layout.h (the workspace carver and the sort-bit helpers): a stand-alone
C++ program built with the address and undefined-behaviour sanitizers. No GPU, no library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_header_host_only(tmp_path):
    """tests/c/layout_check.cpp: a null-base pass and a real pass agree on the size, every array is
    256-B aligned and apart from the others (empty arrays and both floor choices included), and the
    bit-width helpers match their brute-force definitions and minibatch's former 32-bit cap."""
    src = os.path.join(ROOT, "tests", "c", "layout_check.cpp")
    exe = tmp_path / "layout_check"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=undefined", "-g", src, "-o", str(exe)], check=True)
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, (res.returncode, res.stdout[-2000:], res.stderr[-2000:])
    assert "layout ok" in res.stdout


def test_layout_header_is_hip_free():
    """layout.h includes the C++ standard library only, so host-only programs can use it."""
    import re
    text = open(os.path.join(ROOT, "graphconvgeo_amd", "csrc", "layout.h")).read()
    includes = re.findall(r"^\s*#\s*include\s*([<\"][^>\"]+[>\"])", text, flags=re.M)
    assert includes and all(i.startswith("<") and "hip" not in i for i in includes), includes
