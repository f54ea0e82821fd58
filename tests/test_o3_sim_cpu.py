"""The O3 tier's compiled kernels (``mythril_amd/csrc/jit.cpp``: HIP source -> LLVM through comgr)
against the C port on the CPU, in the instruction-level simulator (``tests/asmsim``).

The driver (``asmsim_main.cpp``) compiles each record's kernels itself — ``jit_source`` with
``JIT_SEARCH | JIT_GEN`` and ``jit_compile_local``, so the ``jit.cpp`` under test is this tree's —
and writes the code object (``ASMSIM_O3_DUMP``); ``tools/o3dis.convert`` turns it into text; a second
driver process runs that text per record (``ASMSIM_SEARCH_SOURCE_DIR``) and compares, bit for bit with
the C port (``oracle/bveval.c``) on the unspecialised program: ``mgj_gen`` verdicts per candidate,
``mgj_search`` first hit and hit count with early exit off, first hit and the lowered peer word with
early exit on.

The compile options are the product's defaults, ``-structurizecfg-skip-uniform-regions`` included:
``jit_compile_local`` is the function the product's compile helper calls, and it reads its options
from the same environment variables.  ``test_driver_compiles_what_the_product_compiles`` checks it:
the code object the library's ``mg_program_jit_source`` compiles (kept by ``MYTHGPU_JIT_DUMP``) is
byte for byte the driver's, and ``MYTHGPU_JIT_SKIP_UNIFORM=0`` gives another.

Corpus (``tests/o3_corpus.py``): the table of ``gen_repr_cases`` at its two windows, the GEN3 edge
probes, one program per specialiser-fold family, three fuzz generators (48 programs each, one
unaligned window with bit 31 of the low index word set), the six workloads at two windows.  The table
runs under five configurations of the tier's code-generation switches, one driver process each (they
are read once per process); a configuration must change the emitted source of some table program
(the code object for ``MYTHGPU_JIT_SKIP_UNIFORM``, a compiler option the source does not show).

Conditions: ``outside``, ``simerror``, ``asmerror`` and ``mismatch`` are 0 everywhere.  A program is
left out only if its code object has a private segment (the simulator has no scratch): ``SCRATCH``
lists such programs by name with the segment size, none a workload, at most 5 % of a part.

Teeth: three mutants of ``jit.cpp`` built into the driver each fail the table or the fuzz; the
simulator refuses every modifier its executors do not read (``test_simulator_fails_closed``); every
instruction form this module's change added to the simulator is named with a corpus kernel that
holds it (``FORMS``), so that each stays exercised against the C port.

Wall times of the parts (8 workers): ``profiles/o3_sim_pytest.log``.

Reference anchor: a candidate's verdict is ``Model.eval(And(constraints), model_completion=True)``
(``mythril/laser/smt/model.py:45-59``)."""
import hashlib
import multiprocessing as mp
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import pytest

from tests import o3_corpus as O
from tests.test_asm_sim import ROOT, WORKERS, _mutants, record, run_sim, sim  # noqa: F401  (sim: fixture)

P_ = "MYTHGPU_JIT_"
CONFIGS = {
    "default": {},
    "no_dict_paths": {P_ + "SELECT_DICT": "0", P_ + "DICT_PAIRS": "0", P_ + "DICT_LDS": "0", P_ + "DICT_VEC": "0",
                      P_ + "DELTA_SKIP": "0", P_ + "ALIGNED64": "0"},
    "lane_keys_gate": {P_ + "LANE_KEYS": "1", P_ + "LOOKUP_GATE": "1"},
    "prefetch": {P_ + "PREFETCH": "1"},
    "no_skip_uniform": {P_ + "SKIP_UNIFORM": "0"},
}
# programs whose code object has a private segment {part: {name: bytes}}: left out (no scratch in the simulator)
# (sizes under the default switches; the same two programs under every configuration)
SCRATCH = {"table": {"w256_shift_0": 332, "w256_shift_1": 164}}

# Instruction forms the simulator gained or changed with this module -> a corpus kernel (part,
# configuration, name) whose converted text holds it.
FORMS = {
    r"v_cmp_[lg]t_u32_sdwa .*src[01]_sel:(BYTE|WORD)_0": ("table", "default", "narrow_cmp_3"),  # selects were ignored
    r"v_cmp_\w+_sdwa .*src[01]_sel:(BYTE|WORD)": ("table", "default", "w64_struct_0"),
    r"v_cndmask_b32_sdwa": ("table", "default", "narrow_shift_0"),
    r"v_cndmask_b32_e64 .*\|v\d+\|": ("table", "default", "narrow_div_0"),
    r"v_cndmask_b32_e64 .*-v\d+": ("tier", "default", "tier12"),
    r"v_lshrrev_b32_sdwa": ("tier", "default", "tier11"),
    r"v_sub_u32_e64 .* clamp": ("laser", "default", "laser9"),
    r"s_mov_b64 s\[\d+:\d+\], 0x[89a-f][0-9a-f]{7}$": ("table", "default", "narrow_arith_0"),  # zero-extended
    r"v_writelane_b32": ("table", "default", "narrow_arith_0"),  # SGPR spills: lanes, not registers
    r"v_xnor_b32": ("table", "default", "w64_shift_0"),
    r"v_mul_lo_u16": ("table", "default", "w160_arith_0"),
    r"v_lshrrev_b16": ("table", "default", "w160_arith_0"),
    r"v_mad_legacy_u16": ("table", "default", "w160_arith_0"),
    r"ds_add_u32": ("decided", "default", "decided_laser4"),
    r"v_accvgpr_write_b32": ("table", "default", "narrow_cmp_0"),
    r"v_accvgpr_read_b32": ("table", "default", "narrow_cmp_0"),
    r"v_accvgpr_mov_b32": ("table", "default", "w32_cmp_0"),
    r"ds_read_b\d+ a": ("table", "default", "w160_lookup_0"),
    r"global_load_dword\w* a": ("table", "no_dict_paths", "w160_lookup_0"),
    r"global_load_dwordx3": ("table", "no_dict_paths", "w256_arith_0"),
    r"s_cmpk_gt_u32": ("edge", "default", "edge_mixed"),
    r"s_cmpk_lt_u32": ("edge", "default", "edge_mixed"),
    r"v_bitop3_b16": ("laser", "default", "laser183"),
    r"v_pk_mov_b32 .*op_sel": ("repr", "default", "repr38"),
    # v_mad_u64_u32 with a never-written high addend (its high result then counts as never written)
    r"v_mad_u64_u32": ("table", "lane_keys_gate", "narrow_arith_2"),
}
# the six programs of the issue whose simulated hits differed from the C port's
SIX = {"table": ("narrow_shift_3", "narrow_cmp_3", "w32_struct_0", "w64_struct_0", "w64_struct_1"), "tier": ("tier11",)}
SDWA_CMP_BUG = {"tests/asmsim/asmsim.cpp": (
    "const uint32_t p = enc == 3 ? sdwa(x.lo(l), in.sdwa_sel[0]) : x.lo(l),\n"
    "                         q = enc == 3 ? sdwa(y.lo(l), in.sdwa_sel[1]) : y.lo(l);",
    "const uint32_t p = x.lo(l), q = y.lo(l);")}

# jit.cpp mutants (tests/test_asm_sim._mutants), in the style of test_gen_repr_cpu's
PACKED_BOUND = {"mythril_amd/csrc/jit.cpp": ("if (w > 32 || n == 0 || (uint64_t)n * w > 64) return \"\";",
                                             "if (w > 33 || n == 0 || (uint64_t)n * w > 64) return \"\";")}
# (the delta-skip ballot testing ``cy != 0`` is no mutant: the ballot is wave-wide and running the carry
# chain where no lane needs it changes nothing, so it only skips wrongly when every lane of a wave has
# carry 0 and some lane a negative step with a borrow; it passes table and fuzz, and the hardware would too)
SELECT_LAST = {"mythril_amd/csrc/jit.cpp": ("v = hex(G[off + (n - 1) * L + j]);\n        for (int32_t e",
                                            "v = hex(G[off + 0 * L + j]);\n        for (int32_t e")}
TAIL_GROUP = {"mythril_amd/csrc/jit.cpp": ("const bool full = kk != kpf && kk != kpl;", "const bool full = kk != kpf;")}
# The 64-bit ALIGNED path with its high limb taken from the base alone (the carry of the shifted offset
# into limb 1 dropped).  Table and fuzz never carry there: the edge part's ``edge_aligned`` does, so this
# one is asserted on the edge part.  (The same path taken when the offset reaches three limbs, k == 3,
# fails nothing: no program of the corpus has such a coordinate.  A gap of the case tables, noted in
# README.md.)
ALIGNED_HI = {"mythril_amd/csrc/jit.cpp": (
    r'o << "  " << lim(0) << " = (uint32_t)s64;\n  " << lim(1) << " = (uint32_t)(s64 >> 32); }\n";',
    r'o << "  " << lim(0) << " = (uint32_t)s64;\n  " << lim(1) << " = (uint32_t)(" << base << "ull >> 32); }\n";')}


# ---- one chunk of a part: compile, convert, simulate -----------------------------------------------


def _chunk(args):
    exe, part, lo, hi, env, forms = args
    sys.path.insert(0, str(ROOT))
    from tools.o3dis import convert

    t0 = time.time()
    entries = O.part(part)[lo:hi]
    tmp = Path(tempfile.mkdtemp(prefix="o3sim"))
    try:
        recs = b"".join(record(0, e.pb, e.blob, e.seed, *e.windows[0]) for e in entries)
        rc, summary, lines, err = run_sim(Path(exe), recs, dict(env, ASMSIM_O3_DUMP=str(tmp)))
        out = {"part": part, "compile": (rc, summary, lines[:6], err[-2000:]), "private": {}, "hip": {}, "co": {},
               "forms": {}, "n": 0, "run": None, "names": [e.name for e in entries]}
        if rc or not summary or int(summary["ok"]) != len(entries):
            return out
        priv = {int(m.group(1)): int(m.group(2)) for m in (re.match(r"o3 record (\d+): kernels \d+ private (\d+)", ln)
                                                            for ln in lines) if m}
        run_dir = tmp / "run"
        run_dir.mkdir()
        run = []
        for i, e in enumerate(entries):
            out["hip"][e.name] = hashlib.sha256((tmp / f"{i}.hip").read_bytes()).hexdigest()
            out["co"][e.name] = hashlib.sha256((tmp / f"{i}.co").read_bytes()).hexdigest()
            if priv[i]:
                out["private"][e.name] = priv[i]
                continue
            text = convert(str(tmp / f"{i}.co"))
            out["forms"][e.name] = [f for f in forms if re.search(f, text, re.M)]
            for start, count in e.windows:
                (run_dir / f"{len(run)}.s").write_text(text)
                run.append(record(0, e.pb, e.blob, e.seed, start, count))
        out["n"] = len(run)
        rc, summary, lines, err = run_sim(Path(exe), b"".join(run), dict(env, ASMSIM_SEARCH_SOURCE_DIR=str(run_dir)))
        out["run"] = (rc, summary, lines[:6], err[-2000:])
        out["seconds"] = time.time() - t0
        return out
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


_RUNS = {}


def _run(exe, part, cfg="default", names=None, chunk=4):
    """The part under a configuration: chunks of ``chunk`` programs over ``WORKERS`` processes (cached
    for the unedited driver)."""
    key = (str(exe), part, cfg, names)
    if key in _RUNS:
        return _RUNS[key]
    n = len(O.part(part))
    idx = range(n) if names is None else [i for i, e in enumerate(O.part(part)) if e.name in names]
    spans = []
    for i in idx:  # consecutive indices, `chunk` at most
        if spans and spans[-1][1] == i and i - spans[-1][0] < chunk:
            spans[-1][1] = i + 1
        else:
            spans.append([i, i + 1])
    t0 = time.time()
    tasks = [(str(exe), part, lo, hi, CONFIGS[cfg], tuple(FORMS)) for lo, hi in spans]
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        res = pool.map(_chunk, tasks, chunksize=1)
    print(f"o3 sim: part {part} config {cfg}: {len(idx)} programs, {sum(r['n'] for r in res)} windows, "
          f"{time.time() - t0:.1f} s wall on {WORKERS} workers")
    _RUNS[key] = res
    return res


def _failures(res):
    """records that are not ``ok``, and the compile's / the run's first complaints"""
    bad, why = 0, []
    for r in res:
        rc, summary, lines, err = r["compile"]
        if rc or not summary or r["run"] is None:
            bad += len(r["names"])
            why.append((r["names"], summary, lines, err[-500:]))
            continue
        rc, summary, lines, err = r["run"]
        if not summary:
            bad += r["n"]
            why.append((r["names"], rc, err[-500:]))
            continue
        bad += r["n"] - int(summary["ok"])
        if rc or int(summary["ok"]) != r["n"]:
            why.append((r["names"], summary, lines))
    return bad, why


def _all_ok(part, res, default=True):
    for r in res:
        for rc, summary, lines, err in (r["compile"], r["run"]):
            assert summary, (part, r["names"], rc, err)
            assert all(summary[k] == "0" for k in ("outside", "simerror", "asmerror", "mismatch")) and rc == 0, \
                (part, r["names"], summary, lines, err[-1000:])
        assert int(r["run"][1]["ok"]) == int(r["run"][1]["records"]) == r["n"], (part, r["run"][1])
    private = {k: v for r in res for k, v in r["private"].items()}
    assert sorted(private) == sorted(SCRATCH.get(part, {})) and not (private and part == "workloads"), (part, private)
    if default:
        assert private == SCRATCH.get(part, {}), (part, private)
    assert len(private) <= 0.05 * len(O.part(part)), (part, private)


# ---- the corpus, from the C port alone ---------------------------------------------------------------


def _table_ok(name):
    from tests import gen_repr_cases as G

    c = G.program(name)
    return all(G.window_ok(c, G.seed_of(c), st, n) for st, n in ((G.ALIGNED, G.SIM_COUNT), (G.ODD, G.SIM_COUNT)))


def _fuzz_ok(args):
    part, i = args
    e = O.part(part)[i]
    return all(O.mixed_window(e.pb, e.blob, e.seed, st, n) for st, n in e.windows)


def test_corpus_conditions():
    """Before a tier is looked at: every table window passes ``window_ok``; every fuzz window (512
    unaligned candidates, bit 31 of the low index word set) holds a hit and a miss by the C port;
    the parts have the sizes the module's docstring states."""
    from tests import gen_repr_cases as G

    from oracle import cport

    sizes = {p: len(O.part(p)) for p in O.PARTS}
    for e in O.part("decided"):
        assert cport.search(e.pb, e.blob, e.seed, *e.windows[0])[1] == 0, e.name
    assert sizes["table"] == len(G.program_names()) and sizes["edge"] == 5 and sizes["workloads"] == 6, sizes
    assert all(sizes[p] >= 48 for p in O.FUZZ_PARTS), sizes
    for p in O.FUZZ_PARTS:
        for e in O.part(p):
            (start, count), = e.windows
            assert count == 512 and start & 0x80000000 and start % 64, (e.name, hex(start))
    with mp.get_context("spawn").Pool(WORKERS) as pool:
        assert all(pool.map(_table_ok, G.program_names(), chunksize=4))
        tasks = [(p, i) for p in O.FUZZ_PARTS for i in range(sizes[p])]
        got = pool.map(_fuzz_ok, tasks, chunksize=8)
    assert all(got), [O.part(p)[i].name for (p, i), ok in zip(tasks, got) if not ok]


# ---- the O3 kernels on the simulator -----------------------------------------------------------------


@pytest.mark.parametrize("part", O.PARTS)
def test_part_on_the_simulator(sim, part):  # noqa: F811
    """Every program of the part under the default switches: verdicts, first hit, hit count, early
    exit and the lowered peer word equal the C port's; nothing outside, no simulator or compile error."""
    _all_ok(part, _run(sim, part))


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c != "default"])
def test_table_under_configuration(sim, cfg):  # noqa: F811
    """The table under each configuration of the code-generation switches, and the switch is alive: the
    configuration changes the source of some table program (``no_skip_uniform``: the code object; the
    source is the same by construction, which is asserted too)."""
    res = _run(sim, "table", cfg)
    _all_ok("table", res, default=False)
    base = _run(sim, "table")
    what = "co" if cfg == "no_skip_uniform" else "hip"
    a = {k: v for r in base for k, v in r[what].items()}
    b = {k: v for r in res for k, v in r[what].items()}
    changed = [k for k in a if a[k] != b[k]]
    print(f"o3 sim: configuration {cfg} changes the {what} of {len(changed)} of {len(a)} table programs")
    assert changed, cfg
    if cfg == "no_skip_uniform":
        assert all(r["hip"] == s["hip"] for r, s in zip(base, res))


def test_driver_compiles_what_the_product_compiles(sim, tmp_path):  # noqa: F811
    """The code object of a table program from the library (``native.jit_source(compile=True,
    gen_verdicts=True)``, kept by ``MYTHGPU_JIT_DUMP``: the compile helper, the product's default
    options) is the driver's byte for byte, and so is the source; with ``MYTHGPU_JIT_SKIP_UNIFORM=0``
    both sides give another code object, again the same one."""
    e = O.part("table")[[x.name for x in O.part("table")].index("w64_struct_0")]
    (tmp_path / "pb").write_bytes(e.pb)
    import numpy as np

    np.save(tmp_path / "blob.npy", np.asarray(e.blob, dtype=np.uint32))
    code = ("import numpy as np\nfrom mythril_amd import native\n"
            f"native.jit_source(open({str(tmp_path / 'pb')!r}, 'rb').read(), np.load({str(tmp_path / 'blob.npy')!r}), "
            "compile=True, gen_verdicts=True)\n")
    cos = []
    for k, extra in enumerate(({}, CONFIGS["no_skip_uniform"])):
        d = tmp_path / f"d{k}"
        d.mkdir()
        env = dict(os.environ, MYTHGPU_JIT_DUMP=str(d / "lib"), MYTHGPU_JIT_DISK_CACHE="", **extra)
        subprocess.run([sys.executable, "-c", code], env=env, cwd=str(ROOT), check=True, timeout=300)
        rc, summary, lines, err = run_sim(sim, record(0, e.pb, e.blob, e.seed, *e.windows[0]),
                                          dict(extra, ASMSIM_O3_DUMP=str(d)))
        assert rc == 0, (summary, lines, err)
        assert (d / "lib.hip").read_bytes() == (d / "0.hip").read_bytes()
        assert (d / "lib.co").read_bytes() == (d / "0.co").read_bytes()
        cos.append((d / "0.co").read_bytes())
    assert cos[0] != cos[1]


def test_every_new_simulator_form_is_in_a_corpus_kernel(sim):  # noqa: F811
    """Each instruction form added to or changed in the simulator for the O3 tier's code is held by
    the corpus kernel ``FORMS`` names for it (searched in the converted text), so it is exercised
    against the C port by ``test_part_on_the_simulator``."""
    missing = []
    for form, (part, cfg, name) in FORMS.items():
        res = _run(sim, part, cfg)
        found = {k: v for r in res for k, v in r["forms"].items()}
        if form not in found.get(name, ()):
            missing.append((form, part, name))
    assert not missing, missing


# ---- the simulator refuses what it does not model ----------------------------------------------------

REFUSED = [
    # SDWA selects on an opcode whose executor does not apply them
    "v_bfrev_b32_sdwa v1, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0",
    "v_add_u32_e32 v1, a0, v0",
    "global_load_dword a1, v0, s[0:1]",
    "v_accvgpr_write_b32 v1, v0",
    "v_mov_b32_sdwa v1, v0 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:DWORD",
    "v_cvt_f32_ubyte0_sdwa v1, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_2",
    "v_cmp_eq_u64_sdwa vcc, v[0:1], v[0:1] src0_sel:DWORD src1_sel:DWORD",
    "v_add_u32_e32 v1, v0, v0 src0_sel:BYTE_0",
    "v_add_u32_sdwa v1, v0, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:NIBBLE_0 src1_sel:DWORD",
    "v_add_u32_sdwa v1, sext(v0), v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD",
    "v_cmp_lt_u32_sdwa vcc, v0, v0 dst_sel:BYTE_0 src0_sel:BYTE_0 src1_sel:DWORD",
    "v_not_b32_sdwa v1, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:DWORD src1_sel:BYTE_0",
    "v_mul_lo_u32_sdwa v1, v0, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD",
    # clamp, output modifiers
    "v_and_b32_e64 v1, v0, v0 clamp",
    "v_add_u32_e32 v1, v0, v0 clamp",
    "v_add_u32_e64 v1, v0, v0 clamp",
    "v_mul_f32_e64 v1, -v0, |v0|",
    "v_cvt_f32_ubyte1_e32 v1, v0",
    "v_add_u32_sdwa v1, v0, v0 dst_sel:BYTE_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_0 src1_sel:WORD_1",
    "v_add_u32_sdwa v1, v0, v0 dst_sel:DWORD dst_unused:UNUSED_SEXT src0_sel:BYTE_0 src1_sel:WORD_1",
    "v_xnor_b32_sdwa v1, v0, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:DWORD",
    "v_pk_mov_b32 v[2:3], v[0:1], v[0:1] op_sel_hi:[0,1]",
    "ds_write_b32 v0, a1",
    "v_mad_u32_u24 v1, v0, v0, v0 clamp",
    "v_mul_f32_e64 v1, v0, v0 mul:2",
    "v_mul_f32_e64 v1, v0, v0 div:2",
    # neg / abs where unread
    "v_add_u32_e64 v1, -v0, v0",
    "v_and_b32_e64 v1, |v0|, v0",
    "v_rcp_f32_e64 v1, -v0",
    "v_mul_f32_e32 v1, -v0, v0",
    "v_cndmask_b32_e64 v1, v0, v0, -vcc",
    "v_bfe_u32 v1, v0, -v0, 1",
    # op_sel, DPP
    "v_mad_legacy_u16 v1, v0, v0, v0 op_sel:[1,0,0,0]",
    "v_mov_b32_dpp v1, v0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf",
    "v_add_u32_dpp v1, v0, v0 row_shr:1 row_mask:0xf bank_mask:0xf bound_ctrl:0",
    "v_mov_b32_e32 v1, v0 row_shl:1",
    # memory modifiers on what does not read them
    "v_mov_b32_e32 v1, v0 offset:4",
    "s_mov_b32 s4, 1 offset:4",
    "ds_read_b32 v1, v0 offset0:1",
    "ds_read2_b32 v[2:3], v0 offset:8",
    "ds_read_b32 v1, v0 sc0",
    "v_add_u32_e32 v1, v0, v0 bitop3:0x96",
    "global_load_dword v1, v0, s[0:1] glc",
    "ds_read_b32 v1, v0 gds",
    # encodings an opcode does not have
    "v_bfe_u32_e32 v1, v0, 1, 2",
    "s_mov_b32_e32 s4, 1",
    # a negative literal in a 64-bit scalar operand: the assembler takes it, the hardware zero-extends it
    "s_mov_b64 s[4:5], -14382316",
    "s_mov_b64 s[4:5], 0x1ffffffff",
    # a spill lane read before it was written; an unwritten SGPR through a spill lane, used after the reload
    "v_writelane_b32 v1, s2, 0\n  v_readlane_b32 s4, v1, 1",
    "v_writelane_b32 v1, s9, 0\n  v_readlane_b32 s4, v1, 0\n  s_add_u32 s5, s4, 1",
]
ADMITTED = [  # the same shapes without the token the executor does not read: no refusal
    "v_add_u32_sdwa v1, v0, v0 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:WORD_1",
    "v_cmp_lt_u32_sdwa vcc, v0, v0 src0_sel:BYTE_0 src1_sel:WORD_0",
    "v_sub_u32_e64 v1, v0, v0 clamp",
    "v_cndmask_b32_e64 v1, |v0|, -v0, vcc",
    "s_mov_b64 s[4:5], 0xff248b14",
    "s_mov_b64 s[4:5], -1",
    "v_writelane_b32 v1, s2, 3\n  v_readlane_b32 s4, v1, 3\n  s_add_u32 s5, s4, 1",
    "v_writelane_b32 v1, s9, 0\n  v_readlane_b32 s4, v1, 0",
]


def _one_instruction(sim, tmp_path, k, text):  # noqa: F811
    e = O.part("workloads")[0]
    f = tmp_path / f"k{k}.s"
    f.write_text("mgj_search:\n  v_cmp_eq_u32_e32 vcc, v0, v0\n  s_nop 4\n  " + text + "\n  s_endpgm\n")
    rc, summary, lines, err = run_sim(sim, record(0, e.pb, e.blob, e.seed, 0, 64), {"ASMSIM_SEARCH_SOURCE": str(f)})
    assert summary, (text, rc, err)
    return summary, lines


def test_simulator_fails_closed(sim, tmp_path):  # noqa: F811
    """One-instruction kernels with a modifier token, encoding suffix or select that the opcode's
    executor does not model: a ``SimError`` each (``simerror=1``), never a run.  The admitted
    neighbours of those forms parse and run to the kernel's end."""
    for k, text in enumerate(REFUSED):
        summary, lines = _one_instruction(sim, tmp_path, k, text)
        assert summary["simerror"] == "1" and summary["mismatch"] == "0", (text, summary, lines)
    for k, text in enumerate(ADMITTED):
        summary, lines = _one_instruction(sim, tmp_path, 1000 + k, text)
        assert summary["simerror"] == "0", (text, summary, lines)


# ---- teeth -------------------------------------------------------------------------------------------


def test_the_six_programs_of_the_issue(sim, tmp_path):  # noqa: F811
    """The six programs whose simulated hits differed from the C port's before this module: a
    simulator whose SDWA compares read whole registers again (the selects parsed and dropped, as
    they were) fails each of them, and the unedited simulator passes each.  The first tier emits
    no SDWA compare (its one SDWA form is ``v_xor_b32_sdwa`` with ``src1_sel:WORD_1``, which was
    modelled), so no first-tier test ran through the wrong semantics."""
    exe = _mutants(tmp_path, {"sdwa_cmp": SDWA_CMP_BUG}, o3=True)["sdwa_cmp"]
    for part, names in SIX.items():
        assert _failures(_run(sim, part, names=names, chunk=1))[0] == 0
        res = _run(exe, part, names=names, chunk=1)
        for r in res:
            assert r["run"] and int(r["run"][1]["mismatch"]) >= 1, (r["names"], r["run"])


def test_the_corpus_has_teeth(sim, tmp_path):  # noqa: F811
    """Mutants of ``jit.cpp`` built into the driver — the packed dictionary's width bound off by one,
    the select over a small dictionary's entries ending in entry 0 instead of the last, the
    search kernel's last group of a window taken for a full one (candidates past the end counted) — each fail records of the table or of the
    ``gen_repr`` fuzz that the unedited driver passes; the 64-bit ALIGNED path without its carry into
    the second limb fails the edge part."""
    exes = _mutants(tmp_path, {"packed_bound": PACKED_BOUND, "select_last": SELECT_LAST, "tail_group": TAIL_GROUP,
                               "aligned_hi": ALIGNED_HI}, o3=True)
    for name, exe in exes.items():
        bad = {}
        for part in ("edge",) if name == "aligned_hi" else ("table", "repr"):
            _all_ok(part, _run(sim, part))
            bad[part], why = _failures(_run(exe, part))
        print(f"o3 sim: mutant {name}: records that fail: {bad}")
        assert sum(bad.values()) > 0, name
