"""result_block.h (the block every cohort result lives in) and text_out.h (the two-pass writer of the cohort texts) at their smallest cases:
tests/result_text_unit.cpp, a stand-alone host program over malloc / free, built with the address and undefined-behaviour sanitizers and run
as a child process of its own.  No GPU, no library."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "regtools_amd", "csrc")


def test_result_block_and_text_writer(tmp_path):
    exe = str(tmp_path / "result_text_unit")
    # (the sanitizers' runtimes linked in: the program does not depend on what else its process loads, or in which order)
    build = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-I", CSRC, "-o", exe, os.path.join(HERE, "result_text_unit.cpp")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("result_text_unit ok")
