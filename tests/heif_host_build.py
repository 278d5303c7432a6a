"""Builds tests/heif_host/heif_host.cpp with csrc/host/heif.cpp and nothing else of the product (test infrastructure)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "h264-h265-to-jpeg_amd", "csrc", "host")
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]


def build(tmp, name="heif_host", extra=()):
    """the program's path under the directory `tmp`; extra: more compiler flags (SANITIZE)"""
    exe = str(tmp / name)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++11", "-O1", "-g", "-Wall", "-Wextra", "-I", HOST] + list(extra) +
                          [os.path.join(ROOT, "tests", "heif_host", "heif_host.cpp"), os.path.join(HOST, "heif.cpp"), "-o", exe])
    return exe
