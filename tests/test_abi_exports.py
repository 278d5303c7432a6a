"""The exported symbols of libH265ToJpeg.so against golden/abi/exports.txt: nothing may appear or disappear.

The recording is `nm -D --defined-only` of the library as it was before the host engine was split into modules: the
names of type T, sorted, without the C++ names of namespace h2j (`_ZN3h2j...`, `_ZNK3h2j...`).  Those are the
engine's internal functions, which no header declares and every reorganisation of the host code renames; what
callers link against -- the 51 h2j_* entry points of include/h2j.h, the JNI functions, IDecoder::getInstance and
LOG -- is all in the list.  The price of the filter: an internal function of namespace h2j that starts to be exported,
or stops, goes unnoticed here.
"""
import os
import re
import subprocess

from conftest import PKG, golden


def test_exports_match_recording():
    lib = os.path.join(PKG, "libH265ToJpeg.so")
    assert os.path.exists(lib), f"{lib} is not built: run __graft_entry__.build() first"
    out = subprocess.run(["nm", "-D", "--defined-only", lib], stdout=subprocess.PIPE, check=True).stdout.decode()
    names = sorted(f[2] for f in (l.split() for l in out.splitlines()) if len(f) == 3 and f[1] == "T" and not re.match(r"_ZNK?3h2j", f[2]))
    path = golden(os.path.join("abi", "exports.txt"))
    assert os.path.exists(path), f"{path} is missing: the recording comes from the commit before the refactor"
    with open(path) as f:
        want = f.read().split()
    assert sum(n.startswith("h2j_") for n in want) == 51
    assert names == want, f"appeared: {sorted(set(names) - set(want))}, disappeared: {sorted(set(want) - set(names))}"
