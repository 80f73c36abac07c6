"""The host paths of the C ABI under AddressSanitizer and UBSan: tests/host_paths_check.cpp, a stand-alone program on a backend
without a device (alloc = malloc, launches do nothing), goes through every description model creation refuses, walks model and batch
creation (one, two and three body shapes), the setters, ss_imitation_bind and the teardown, then repeats the walk with the n-th
allocation or upload failing, for every n.  A leak, a double free or undefined
behaviour on any of those paths fails the run.

Cost: the program stays off ss_kernel.h; g++ with both sanitizers takes about 20 s on it (ss_mjcf.h and ss_tables.h are most of
that) and the 32 walks about 5 s, against about 50 s for the emulator's normal build on the same machine."""
import gzip
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_host_paths_are_clean_under_asan_and_ubsan(tmp_path):
    exe, xml = str(tmp_path / "host_paths_check"), str(tmp_path / "smpl_humanoid.xml")
    with gzip.open(os.path.join(ROOT, "tests", "golden", "mjcf", "smpl_humanoid.xml.gz"), "rb") as f, open(xml, "wb") as g:
        g.write(f.read())
    # the sanitizers' runtimes are linked statically into the program: nothing is loaded into Python, nothing is preloaded
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "host_paths_check.cpp"), "-o", exe])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, xml], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(r.stdout)
    assert r.returncode == 0 and "Sanitizer" not in r.stdout and "runtime error" not in r.stdout, r.stdout
    m = re.search(r"(\d+) allocations and uploads in the full run, (\d+) failing runs", r.stdout)
    assert m and int(m.group(1)) == int(m.group(2)) >= 36          # every allocation and upload failed once (three models alone: six tables each, allocated and uploaded)
