"""The decoder's routes, pinned on the CPU: which kernel decodes the units, what runs in front of it, with which arguments.

tests/dec_route_harness.cpp links the host half of the decoder (k_host.o, k_dec_launch.o, k_dec_win.o) against recorders in
place of the kernel launchers and of HIP, and calls launch_decode over a grid of rasters, tables, alignments, walk memory and
strips.  The debugging switches are read once per process, so every switch setting is a run of its own.  Two fixtures:

  tests/golden/dec_routes.fnv   an FNV-1a64 of the complete output per (switch, value size, mode): pins every case of the grid
  tests/golden/dec_routes.txt   one readable case per distinct launch sequence (names, scopes, which of bl_mode / totals_only /
                                from_ix / chk_wgs are set), the first the grid meets: what to read when a hash changes

Both were made from the objects of the commit before the launch code was restated (the command is in that commit's message);
`python tests/test_decode_routes.py --write [OBJECT_DIR]` writes them again from the objects in OBJECT_DIR (default: the build's).
No device is needed or touched.
"""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "qb3_amd", "csrc")
GOLDEN = os.path.join(ROOT, "tests", "golden")
HIPCC = shutil.which("hipcc") or ("/opt/rocm/bin/hipcc" if os.path.exists("/opt/rocm/bin/hipcc") else None)
OBJECTS = ["k_host", "k_dec_launch", "k_dec_win"]
SWITCHES = [("none", {}), ("QB3_NO_PX", {"QB3_NO_PX": "1"}), ("QB3_SLOW_WALK", {"QB3_SLOW_WALK": "1"}), ("QB3_SLOW_INDEX", {"QB3_SLOW_INDEX": "1"}),
            ("QB3_NO_BLOCK_LENGTHS", {"QB3_NO_BLOCK_LENGTHS": "1"}), ("QB3_WALK_TAB_KB=2048", {"QB3_WALK_TAB_KB": "2048"}),
            ("QB3_WIDE_BAND=17", {"QB3_WIDE_BAND": "17"}), ("QB3_EXITS_FROM=0", {"QB3_EXITS_FROM": "0"})]


def _objects(objdir, must_exist):
    """the host objects the harness links; with must_exist, those the build has not left are made now (make, as the build makes them)"""
    paths = [os.path.join(objdir, n + ".o") for n in OBJECTS]
    missing = [p for p in paths if not os.path.exists(p)]
    if missing and must_exist:
        subprocess.run(["make", "-C", CSRC, "ARCH=gfx950"] + [os.path.join("build", os.path.basename(p)) for p in missing], check=True, capture_output=True)
        missing = []
    return [p for p in paths if p not in missing]


def _build(objs, workdir, source=os.path.join(ROOT, "tests", "dec_route_harness.cpp"), include=CSRC):
    exe = os.path.join(workdir, "dec_route_harness")
    subprocess.run([HIPCC, "-x", "hip", "--cuda-host-only", "-O2", "-std=c++17", "-fPIC", "-I", include, "-c", source, "-o", exe + ".o"], check=True, capture_output=True)
    subprocess.run(["g++", exe + ".o"] + objs + ["-o", exe, "-lpthread"], check=True, capture_output=True)      # (no HIP runtime: every entry point is the harness's)
    return exe


def _signature(block):
    sig = []
    for line in block.splitlines()[3:]:
        f = line.split()
        m = re.search(r"bl_mode=(\d+) totals_only=(\d+) chk_wgs=(\d+) from_ix=(\d+)", line)
        sig.append(f[0] + " " + ("".join("0" if v == "0" else "1" for v in m.groups()) if m else " ".join(f[1:] if f[0] in ("{", "->") else [])))
    return "\n".join(sig)


def run_all(objs, workdir, mode=(), switches=None, signature=None, exe=None):
    """(text of dec_routes.fnv, text of dec_routes.txt) from one run of the harness per switch setting, all at once.  With a mode, switches
    and a signature of its own tests/test_encode_routes.py gets the encoder's two texts from here; run I's whole output stays in
    workdir/runI.txt"""
    switches, signature = switches or SWITCHES, signature or _signature
    exe = exe or _build(objs, workdir)
    base = {k: v for k, v in os.environ.items() if not k.startswith("QB3_")}
    logs = [open(os.path.join(workdir, "run%d.txt" % i), "w+") for i in range(len(switches))]      # (files, not pipes: no run waits for a reader)
    procs = [subprocess.Popen([exe] + list(mode) + [name], env=dict(base, **env), stdout=log) for (name, env), log in zip(switches, logs)]
    fnv, routes, seen = [], [], set()
    for (name, _), p, log in zip(switches, procs, logs):
        assert p.wait() == 0, "the harness failed under switch %s" % name
        log.seek(0)
        out = log.read()
        log.close()
        fnv += [line for line in out.splitlines() if line.startswith("fnv ")]
        routes.append("## switch %s: the launch sequences no setting above has shown\n" % name)
        for block in out.split("\n\n"):
            if block.startswith("case ") and signature(block) not in seen:
                seen.add(signature(block))
                routes.append(block + "\n")
    return "\n".join(fnv) + "\n", "\n".join(routes)


@pytest.fixture(scope="module")
def outputs(tmp_path_factory):
    return run_all(_objects(os.path.join(CSRC, "build"), True), str(tmp_path_factory.mktemp("routes")))


needs_hipcc = pytest.mark.skipif(HIPCC is None, reason="no hipcc: the harness includes the kernels' argument blocks")


@needs_hipcc
def test_every_route_of_the_grid(outputs):
    with open(os.path.join(GOLDEN, "dec_routes.fnv")) as f:
        want = f.read()
    got = outputs[0]
    changed = [a + "   was   " + b for a, b in zip(got.splitlines(), want.splitlines()) if a != b]
    assert got == want, "the decoder takes another route, or launches with other arguments, in:\n" + "\n".join(changed)


@needs_hipcc
def test_distinct_launch_sequences(outputs):
    with open(os.path.join(GOLDEN, "dec_routes.txt")) as f:
        want = f.read()
    assert len(want) <= 200 * 1024
    assert outputs[1] == want


if __name__ == "__main__":
    import tempfile
    if len(sys.argv) < 2 or sys.argv[1] != "--write":
        sys.exit("usage: test_decode_routes.py --write [OBJECT_DIR]")
    objdir = sys.argv[2] if len(sys.argv) > 2 else os.path.join(CSRC, "build")
    with tempfile.TemporaryDirectory() as tmp:
        fnv_text, routes_text = run_all(_objects(objdir, False), tmp)
    for fname, text in (("dec_routes.fnv", fnv_text), ("dec_routes.txt", routes_text)):
        with open(os.path.join(GOLDEN, fname), "w") as f:
            f.write(text)
    print("wrote %d hashes, %d bytes of routes" % (fnv_text.count("\n"), len(routes_text)))
