"""The calls of test_heif_handover.py, run in a fresh child python against the host-memory stand-in for libh2j_hip.so
(see handover_cases.py: same conventions).  Everything goes to stderr: a `== label` line per call, the stand-in's
transcript of the call, and a `result` line (JSON)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "h264-h265-to-jpeg_amd"))

import handover_cases as H  # noqa: E402
import heif_mux as M  # noqa: E402

STREAMS = [("hevc/p11_64x64_tiny.h265", 265), ("h264/a11_64x64_tiny.h264", 264), ("hevc/p19_480x272_tiles2x2_wpp_nolf.h265", 265)]


def main():
    import h2j
    h2j.load_library()
    for name, codec in STREAMS:
        with open(os.path.join(H.GOLDEN, name), "rb") as f:
            s = f.read()
        heic = M.mux([s], codec=codec, iloc_version=1, construction=1, thumb=True)
        for label, batch in (("annexb twice", [s, s]), ("annexb and heic", [s, heic]), ("heic twice", [heic, heic])):
            e = H.fresh()
            H.say(f"== {name}: {label}")
            out = e.transcode(batch)
            H.result(status=e.last_status, sof=[H.sof_size(j) for j in out])


if __name__ == "__main__":
    main()
