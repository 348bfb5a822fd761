"""CPU suite: the plan validator under the address and undefined-behaviour sanitizers, in a stand-alone program.

The ctypes tests of tests/test_plan_validation.py see what ``ctg_plan_create`` answers, not whether it stayed inside the
blob -- or inside 64 bits -- while it judged.  tests/cabi_validate_fuzz.cpp is a program with its own ``main`` that links
the library's objects, csrc/ctg_runtime.hip and csrc/ctg_lds_host.hip compiled with ``-fsanitize=address,undefined`` on
the host side (the build()'s variant mechanism; device code as always): the sanitizer runtime comes from the
executable, nothing is preloaded.  It replays the mutation list of tests/test_plan_validation.py on every fixture, adds
seeded random mutants of one to four words, and runs every accepted plan through the plan queries and every host
function that reads a plan's tables at executor creation.  It makes no ``ctg_exec_*`` call and no HIP call, and this
test is not a GPU test: a mutated plan never reaches an executor or a device.
"""
import os
import subprocess

import numpy as np

import test_plan_validation as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN_FLAGS = ("-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-g")
SAN_SOURCES = ["ctg_runtime.hip", "ctg_lds_host.hip"]
# Random mutants per fixture.  Sized by time, not by count: with the 11 373 listed mutants of the twelve fixtures, 12 x
# 10 000 random ones take the sanitized program about 20 s on the development machine (12 x 4 000 took 9 s; a mutant
# costs 0.1-0.2 ms: a copy of the plan, ctg_plan_create, and for the accepted ones the host readers).  Fixed seed: the
# same mutants every run.
RANDOM_PER_FIXTURE = 10000
SEED = 20240607
MAGIC = 0x43544750


def build_program():
    """The sanitized objects (rebuilt when out of date, as build() rebuilds everything) and the program linked on them."""
    import __graft_entry__ as ge

    libdir = os.path.join(ROOT, "cotengra_amd", "lib", "exp")
    os.makedirs(libdir, exist_ok=True)
    ge.build(extra_flags=SAN_FLAGS, lib=os.path.join(libdir, "libctg_validate_san.so"), flag_sources=SAN_SOURCES)
    tag = "".join(c if c.isalnum() else "_" for c in " ".join(SAN_FLAGS))
    objs = [os.path.join(ge.OBJ, tag if s in SAN_SOURCES else "default", os.path.splitext(s)[0] + ".o") for s in ge.SOURCES]
    assert all(os.path.exists(o) for o in objs)
    src, exe = os.path.join(ROOT, "tests", "cabi_validate_fuzz.cpp"), os.path.join(libdir, "cabi_validate_fuzz")
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(map(os.path.getmtime, objs + [src])):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
        # (the program is plain C++: compiled as such, then linked by the HIP driver with the library's objects)
        subprocess.run([hipcc, "-O1", "-g", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-x", "c++", "-c", src,
                        "-o", exe + ".o"] + san, check=True)
        subprocess.run([hipcc, "--offload-arch=gfx950", "-o", exe, exe + ".o"] + objs + san + ["-ldl"], check=True)
    return exe


def write_fixture(fx, path):
    """The plan in the word layout of tests/golden/gen/make_cabi_plan.py, the group flags, the mutation list."""
    f = fx.f
    head = [MAGIC, f["dtype"], fx.n_inputs, f["inputs_elems"], f["arena_elems"], f["result_elems"], fx.n_steps, fx.blob,
            fx.n_sliced, fx.base[2]]
    words = [np.array(head, dtype="<i8")] + [f[k].astype("<i8") for k in ("input_sizes", "input_offsets", "steps", "tables",
                                                                        "slice_sizes", "slice_fixed", "slice_strides", "slice_group")]
    rows = V.rows_of(fx)
    mut = [len(rows)]
    for _, edits, expect in rows:
        mut += [1 if expect == "accept" else 0, len(edits)]
        for field, idx, val in edits:
            mut += [V.FIELDS.index(field), idx, val]
    words.append(np.array(mut, dtype="<i8"))
    with open(path, "wb") as out:
        for w in words:
            out.write(np.ascontiguousarray(w).tobytes())
    return len(rows)


def test_validator_is_clean_under_the_sanitizers(tmp_path):
    exe = build_program()
    files, listed = [], 0
    for name in V.FIXTURE_NAMES:
        files.append(str(tmp_path / (name + ".plan")))
        listed += write_fixture(V.fixtures()[name], files[-1])
    env = dict(os.environ)
    env["ASAN_OPTIONS"] = "detect_leaks=1:abort_on_error=0"
    env["UBSAN_OPTIONS"] = "print_stacktrace=1:halt_on_error=1"
    p = subprocess.run([exe, str(RANDOM_PER_FIXTURE), str(SEED)] + files, capture_output=True, text=True, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    assert "Sanitizer" not in p.stderr and "runtime error" not in p.stderr, p.stderr[-6000:]
    assert p.stdout.startswith(f"replayed {listed} listed and {RANDOM_PER_FIXTURE * len(files)} random mutants"), p.stdout
