"""The SEI walker (bitstream.cpp sei_display_orientation, stream_display_orientation) over malformed input under
AddressSanitizer and UndefinedBehaviorSanitizer: host code only, in a stand-alone program with its own main
(tests/sei_walk/sei_walk_case.cpp) whose buffers are heap blocks of exactly the input's size, so a read past the
NAL unit is a report.  The sanitizer runtimes are linked into the program.  No GPU, nothing loaded into Python."""
import os
import subprocess

from conftest import PKG, ROOT


def test_sei_walker_reads_nothing_past_the_nal(tmp_path):
    exe = str(tmp_path / "sei_walk_case")
    host = os.path.join(PKG, "csrc", "host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", "-I" + host, "-o", exe,
                           os.path.join(ROOT, "tests", "sei_walk", "sei_walk_case.cpp"), os.path.join(host, "bitstream.cpp")])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.stdout.decode()[-500:], out.stderr.decode()[-3000:])
    words = out.stdout.decode().split()
    assert words[0] == "walked" and int(words[1]) > 200000, out.stdout
