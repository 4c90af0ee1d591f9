"""The launch-table cache of a context (homulator_amd/csrc/hm_table_cache.h: what device_table in hm_backend.hip instantiates with the HIP calls)
on the CPU, no GPU: tests/emu/hm_table_cache_main.cpp instantiates it with malloc / memcpy / free and replays calls that keep earlier device
pointers inside later tables.  A stand-alone program with its own main, compiled with the sanitizers and run as a process of its own (nothing is
loaded into Python): a table freed before the call that obtained it has returned is a heap-use-after-free where the call reads it."""
import os
import re
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_stand_alone_program_under_the_sanitizers(tmp_path):
    exe = tmp_path / "hm_table_cache_main"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           "-o", str(exe), os.path.join(HERE, "emu", "hm_table_cache_main.cpp")])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "bad=0" in r.stdout, r.stdout + r.stderr
    m = re.search(r"calls=(\d+) evictions_unpinned=(\d+)", r.stdout)
    assert m and int(m.group(1)) > 1000 and int(m.group(2)) > 0, r.stdout   # the sweep ran, and it evicted
