"""The error bound of the sequential float sum that rtcsm_bounds_kernel widens every candidate's score interval by
(d-liom_amd/csrc/rtcsm_bounds.h): the kernel looks it up in a table of one double per binade of U, filled on the host
once a match, where every candidate used to run the loop of up to 68 ldexp / floor / divisions itself.

Without a GPU: tests/cpp/rtcsm_bound_table_check.cc holds the look-up against the loop on the doubles' bits, for
n = 1, 64, 170, 65 536, 262 144 and 2^19 and U at both ends and in the middle of every binade from 2^-4 to 2^20 (and
the corners outside); built with the library's host flags and once more, stand-alone, with -fsanitize=address,undefined."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHECK = os.path.join(ROOT, "tests", "cpp", "rtcsm_bound_table_check.cc")
CASES = 6 * (25 * 4 + 13)  # six cloud sizes; four doubles in each of the 25 binades, thirteen corners


def _build_and_run(tmp_path, name, flags):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror"] + flags + ["-o", exe, CHECK])
    out = subprocess.check_output([exe]).decode().split()
    print(" ".join(out))
    return out


def test_bound_table_equals_the_loop(tmp_path):
    out = _build_and_run(tmp_path, "rtcsm_bound_table_check", ["-O3"])
    assert out == ["ok", "cases", str(CASES)]


def test_bound_table_under_sanitizers(tmp_path):
    out = _build_and_run(tmp_path, "rtcsm_bound_table_check_san",
                         ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    assert out == ["ok", "cases", str(CASES)]
