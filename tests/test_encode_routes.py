"""The encoder's routes, pinned on the CPU: which kernel codes the units, with which plan and which arguments.

The `enc` mode of tests/dec_route_harness.cpp records the encoder's launchers instead of refusing them, and calls launch_encode,
launch_encode_strip and launch_encode_tail over a grid of rasters, band maps, curves, image pointers, tile batches, indexes, tables
and probes; value_aligned is what the two callers of plan_encode would compute from the case's pointer and pitches.  plan_encode
reads one debugging switch, QB3_NO_PX, so there are two runs.  Two fixtures, in the scheme of tests/test_decode_routes.py (whose
build and run helpers this file uses):

  tests/golden/enc_routes.fnv   an FNV-1a64 of the complete output per (switch, value size, mode): pins every case of the grid
  tests/golden/enc_routes.txt   one readable case per distinct launch sequence (launchers, front end, scope, finish_what, ix_coder,
                                have_idx, idx_no_ulen), the first the grid meets: what to read when a hash changes

Both were made from the objects of the commit before the encoder's kernel became one choice (EncKernel), with a copy of the harness
that spoke that commit's interface (how: that commit's message); `python tests/test_encode_routes.py --write [OBJECT_DIR [HARNESS]]`
writes them again from the objects in OBJECT_DIR (default: the build's; headers from the directory above it) and the harness source
HARNESS (default: this tree's).  No device is needed or touched.

What no earlier state of the code can show is asserted here directly: a plan made for value-aligned memory and launched with other
memory is refused before anything is launched.
"""
import os
import re
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_decode_routes as R  # noqa: E402

SWITCHES = [("none", {}), ("QB3_NO_PX", {"QB3_NO_PX": "1"})]
FIELDS = re.compile(r" ix_coder=(\d+) .* have_idx=(\d+) idx_no_ulen=(\d+) .* finish_what=(\d+)")
FRONT = re.compile(r" front=(\d+)")


def _signature(block):
    sig = []
    for line in block.splitlines()[2:]:
        f = line.split()
        m = FIELDS.search(line)
        sig.append(f[0] + " " + (" ".join(FRONT.findall(line) + list(m.groups())) if m else " ".join(f[1:])))
    return "\n".join(sig)


def run_all(objs, workdir, exe=None):
    return R.run_all(objs, workdir, mode=("enc",), switches=SWITCHES, signature=_signature, exe=exe)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    workdir = str(tmp_path_factory.mktemp("enc_routes"))
    fnv, routes = run_all(R._objects(os.path.join(R.CSRC, "build"), True), workdir)
    with open(os.path.join(workdir, "run0.txt")) as f:
        refusals = [line for line in f.read().splitlines() if line.startswith("refusal ")]
    return fnv, routes, refusals


needs_hipcc = R.needs_hipcc


@needs_hipcc
def test_every_route_of_the_grid(outputs):
    with open(os.path.join(R.GOLDEN, "enc_routes.fnv")) as f:
        want = f.read()
    got = outputs[0]
    changed = [a + "   was   " + b for a, b in zip(got.splitlines(), want.splitlines()) if a != b]
    assert got == want, "the encoder takes another kernel, or launches with another plan or other arguments, in:\n" + "\n".join(changed)


@needs_hipcc
def test_distinct_launch_sequences(outputs):
    with open(os.path.join(R.GOLDEN, "enc_routes.txt")) as f:
        want = f.read()
    assert len(want) <= 200 * 1024
    assert outputs[1] == want


@needs_hipcc
def test_a_plan_that_does_not_fit_the_memory_is_refused(outputs):
    """px16, pxw and best_front, each planned for value-aligned memory: launched at an odd pointer, and at an aligned pointer with an odd
    tile pitch, launch_encode returns nonzero, no launcher is reached and last_error names the alignment"""
    got = [dict(x.split("=", 1) for x in line.split(" ", 6)[1:]) for line in outputs[2]]
    assert [(r["kernel"], r["memory"]) for r in got] == [(k, m) for k in ("px16", "pxw", "best_front") for m in ("odd_pointer", "odd_pitch")]
    for r in got:
        assert r["planned"] == "1", "plan_encode no longer chooses %s for this raster" % r["kernel"]
        assert int(r["rc"]) != 0 and r["records"] == "0" and "value-aligned memory" in r["error"], r


if __name__ == "__main__":
    import tempfile
    if len(sys.argv) < 2 or sys.argv[1] != "--write":
        sys.exit("usage: test_encode_routes.py --write [OBJECT_DIR [HARNESS]]")
    objdir = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 else os.path.join(R.CSRC, "build")
    with tempfile.TemporaryDirectory() as tmp:
        objs = R._objects(objdir, False)
        exe = R._build(objs, tmp, sys.argv[3], os.path.dirname(objdir)) if len(sys.argv) > 3 else None
        fnv_text, routes_text = run_all(objs, tmp, exe)
    for fname, text in (("enc_routes.fnv", fnv_text), ("enc_routes.txt", routes_text)):
        with open(os.path.join(R.GOLDEN, fname), "w") as f:
            f.write(text)
    print("wrote %d hashes, %d bytes of routes" % (fnv_text.count("\n"), len(routes_text)))
