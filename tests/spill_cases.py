"""The first tier's LDS spiller at its thresholds (``jit_asm.cpp``, ``Gen::spill_one`` / ``reload``):
the programs of ``tests/test_asm_spill_sim.py`` (CPU) and ``tests/test_gpu_asm_spill.py`` (GPU).

The family is the many-key read of ``test_asm_eval_spills_sim``: a weighted sum over
``select(arr, k_i)`` at ``keys`` distinct symbolic keys of ``width`` bits.  Every lookup compares its
key with every earlier one, so all keys stay live to the last lookup, ``ceil(width / 32)`` VGPRs
each, and the live limbs past the register file go to LDS slots.  The model read-back rows
(``search.model_watch``: every key and every byte read) are watched, and after them the XOR of all
keys.  The kernel stores a key's own watch rows where it loads the key, before any spill, and two
random wide keys never compare equal, so without the XOR no output of a 256-bit case depends on
what a reload brings back; the XOR reads every key once more after the last lookup, and a limb
reloaded from the wrong slot shows in its rows.

An eval kernel is of one of four classes:

* ``resident``: nothing spills;
* ``four-wave``: the four waves of a workgroup each hold ``stride`` slots (``stride`` = the
  high-water mark made odd), at most 159: 4 x 159 x 256 B = 162,816 B of the CU's 163,840;
* ``solo``: one working wave per workgroup, at most 639 slots, one 64-candidate group per workgroup
  and no group loop.  A kernel goes solo when its four-wave attempt needs a 160th slot, or when
  its body may be longer than the group loop's branches span (32,767 dwords): with the model rows
  watched the second happens first at every width but 256, which the table says per case (a solo
  kernel with a mark of 159 or less went solo for its length);
* ``refused``: past the solo cap, ``EngineUnsupported`` (out of spill slots).

Each program is compiled row-major and tiled; the two kernels allocate differently, so a case
declares a class and, where it matters, a high-water mark per layout.  The key counts were found
by sweeping with the real 256-register file and will move when the emitter changes: the tests
read class and mark from the emitted text and fail on a count that no longer stands where the
table says (``ROLES`` below), which is the signal to sweep again.

Two marks no program of this family reaches with four waves and the full register file:

* a four-wave kernel at mark 159, the largest legal one.  Marks move in steps of the keys' limbs and
  only 96-bit keys reach 159 (at 97 keys), in a body long past the branch range.  ``w96_k57_r97``
  reaches it with 57 keys, a 97-register file (``MYTHGPU_JIT_ASM_SPILL_TEST``) and only the sum
  watched (the model rows and the XOR would put that body past the branch range as well);
* a solo attempt that needs exactly 640 comes from 256-bit keys (marks in steps of 8): 95 keys
  stop at 632, 96 keys need 640 and are refused.  Mark 639 itself is 217 keys of 96 bits (a kernel of
  about 297,000 lines that assembles and passes the load gate), 218 are refused.
"""
import functools
import random
import re
from typing import NamedTuple, Optional

WIDTHS = (64, 96, 128, 160, 256)
LDS_PER_CU = 160 * 1024
FOUR_WAVE_CAP, SOLO_CAP = 159, 639
SOLO_MARKER = "mgj_meta_eval_cpb:"

RESIDENT, FOUR_WAVE, SOLO, REFUSED = "resident", "four-wave", "solo", "refused"


class Case(NamedTuple):
    width: int
    keys: int
    row: str                       # the row-major kernel's class
    tiled: str                     # the tiled kernel's class
    roles: tuple = ()              # what the case stands for (ROLES)
    row_hwm: Optional[int] = None  # the high-water mark the role needs, per layout (None: any)
    tiled_hwm: Optional[int] = None
    regs: Optional[int] = None     # MYTHGPU_JIT_ASM_SPILL_TEST (None: the real register file)
    watch: str = "model"           # "model": the model read-back rows; "sum": the sum alone

    @property
    def name(self) -> str:
        return f"w{self.width}_k{self.keys}" + (f"_r{self.regs}" if self.regs else "_sum" if self.watch == "sum" else "")

    def cls(self, tiled: bool) -> str:
        return self.tiled if tiled else self.row

    def hwm(self, tiled: bool) -> Optional[int]:
        return self.tiled_hwm if tiled else self.row_hwm

    @property
    def env(self) -> dict:
        return {"MYTHGPU_JIT_ASM_SPILL_TEST": str(self.regs)} if self.regs else {}


# What test_spill_table_holds_the_thresholds asks of the table, read from the emitted text:
#   last-resident / first-spill    per width, keys k and k + 1: resident, then spilling (both layouts)
#   last-four-wave / first-solo    per width and layout, keys k and k + 1 (":row" / ":tiled")
#   hwm-159                        a four-wave kernel at the largest legal mark
#   needs-160                      a kernel at mark 160: its four-wave attempt was refused, solo
#   past-160                       the first solo kernel past a needs-160 one (keys + 1)
#   hwm-639 / past-639             the solo cap: the largest legal mark, and one more key (refused)
#   needs-640                      keys k (solo) and k + 1 (refused) of 256 bits: marks 632 and 640
#   boundary                       also through comgr in the simulator run, and on the GPU
CASES = (
    # 64-bit keys (2 limbs): the body passes the branch range at 85 keys, long before the slots run out
    Case(64, 77, RESIDENT, RESIDENT, ("last-resident",)),
    Case(64, 78, FOUR_WAVE, FOUR_WAVE, ("first-spill",)),
    Case(64, 84, FOUR_WAVE, FOUR_WAVE, ("last-four-wave:row", "boundary")),
    Case(64, 85, SOLO, FOUR_WAVE, ("first-solo:row", "boundary")),
    Case(64, 86, SOLO, FOUR_WAVE, ("last-four-wave:tiled",)),
    Case(64, 87, SOLO, SOLO, ("first-solo:tiled",)),
    Case(64, 130, SOLO, SOLO, ("needs-160",), row_hwm=160),
    Case(64, 131, SOLO, SOLO, ("past-160",)),
    # 96-bit keys (3 limbs)
    Case(96, 58, RESIDENT, RESIDENT, ("last-resident",)),
    Case(96, 59, FOUR_WAVE, FOUR_WAVE, ("first-spill",)),
    Case(96, 71, FOUR_WAVE, FOUR_WAVE, ("last-four-wave:row", "boundary")),
    Case(96, 72, SOLO, FOUR_WAVE, ("first-solo:row", "last-four-wave:tiled", "boundary")),
    Case(96, 73, SOLO, SOLO, ("first-solo:tiled",)),
    Case(96, 57, FOUR_WAVE, FOUR_WAVE, ("hwm-159", "boundary"), row_hwm=159, tiled_hwm=159, regs=97, watch="sum"),
    Case(96, 217, SOLO, SOLO, ("hwm-639",), row_hwm=639, tiled_hwm=639),
    Case(96, 218, REFUSED, REFUSED, ("past-639",)),
    # 128-bit keys (4 limbs)
    Case(128, 46, RESIDENT, RESIDENT, ("last-resident",)),
    Case(128, 47, FOUR_WAVE, FOUR_WAVE, ("first-spill",)),
    Case(128, 61, FOUR_WAVE, FOUR_WAVE, ("last-four-wave:row", "boundary")),
    Case(128, 62, SOLO, FOUR_WAVE, ("first-solo:row", "last-four-wave:tiled", "boundary")),
    Case(128, 63, SOLO, SOLO, ("first-solo:tiled",)),
    Case(128, 78, SOLO, SOLO, ("needs-160",), tiled_hwm=160),
    Case(128, 79, SOLO, SOLO, ("past-160",)),
    # 160-bit keys (5 limbs)
    Case(160, 38, RESIDENT, RESIDENT, ("last-resident",)),
    Case(160, 39, FOUR_WAVE, FOUR_WAVE, ("first-spill",)),
    Case(160, 54, FOUR_WAVE, FOUR_WAVE, ("last-four-wave:row", "boundary")),
    Case(160, 55, SOLO, FOUR_WAVE, ("first-solo:row", "last-four-wave:tiled", "boundary")),
    Case(160, 56, SOLO, SOLO, ("first-solo:tiled",)),
    Case(160, 64, SOLO, SOLO, ("needs-160",), row_hwm=160),
    Case(160, 65, SOLO, SOLO, ("past-160",)),
    # 256-bit keys (8 limbs): the one width whose four-wave kernels end at the slot cap, not at the
    # branch range.  42 keys, row-major, is the kernel that declared 164,864 B before the cap bounded
    # the stride; tiled, 42 keys stop at mark 152 and 43 need 168
    Case(256, 25, RESIDENT, RESIDENT, ("last-resident",)),
    Case(256, 26, FOUR_WAVE, FOUR_WAVE, ("first-spill",)),
    Case(256, 41, FOUR_WAVE, FOUR_WAVE, ("last-four-wave:row", "boundary")),
    Case(256, 42, SOLO, FOUR_WAVE, ("first-solo:row", "last-four-wave:tiled", "needs-160", "boundary"), row_hwm=160),
    Case(256, 43, SOLO, SOLO, ("first-solo:tiled", "past-160", "boundary")),
    # the same with the sum alone watched, a body of 14,800 lines well inside the branch range: nothing
    # but the slot cap stands between this program and a four-wave kernel of 164,864 B
    Case(256, 42, SOLO, SOLO, ("needs-160", "boundary"), row_hwm=160, tiled_hwm=160, watch="sum"),
    Case(256, 43, SOLO, SOLO, ("past-160",), watch="sum"),
    Case(256, 95, SOLO, SOLO, ("needs-640",), row_hwm=632, tiled_hwm=632),
    Case(256, 96, REFUSED, REFUSED, ("needs-640",)),
)

BOUNDARY = tuple(c for c in CASES if "boundary" in c.roles)


def by_role(role: str):
    return [c for c in CASES if role in c.roles]


def many_key_terms(width: int, keys: int):
    """(roots, sum, keys, reads, fold): the weighted sum over ``select(arr, k_i)`` of ``keys`` symbolic
    keys, and the XOR of all keys, which reads every key once more after the last lookup."""
    from mythril_amd.smt import terms as T

    arr = T.ArrayVar("Cd", width, 8)
    acc = T.BitVecVal(0, 32)
    rng = random.Random(3)
    ks, reads = [], []
    for i in range(keys):
        ks.append(T.BitVecVar(f"k{i}", width))
        reads.append(T.select(arr, ks[-1]))
        acc = T.bvbin("bvadd", acc, T.bvbin("bvmul", T.zero_extend(24, reads[-1]), T.BitVecVal(rng.getrandbits(32), 32)))
    fold = ks[0]
    for k in ks[1:]:
        fold = T.bvbin("bvxor", fold, k)
    return [T.eq(T.extract(2, 0, acc), T.BitVecVal(5, 3))], acc, ks, reads, fold


@functools.lru_cache(maxsize=None)
def program(case: Case):
    """(the flattened program, its serialised bytes).  Watched (``model``): what ``search.model_watch``
    reads back — every key, then per array site its key and the byte read — with each site's base
    value (``0x80000000 | coordinate``, which the C port does not evaluate) spelt as the select's own
    node: the same value, no store lies between.  Watched last in both forms: the XOR of all keys."""
    from mythril_amd import search, ssa

    roots, acc, ks, reads, fold = many_key_terms(case.width, case.keys)
    P = ssa.flatten(roots, extra=[fold])
    node = lambda t: P.term_node[t.id]  # noqa: E731
    if case.watch == "model":
        watch = [node(k) for k in ks] + [node(t) for k, r in zip(ks, reads) for t in (k, r)]
        assert len(watch) == len(search.model_watch(P)[0])
        watch.append(node(fold))
    else:
        watch = [node(acc)]
    P.set_watch(watch)
    return P, P.to_bytes()


class Facts(NamedTuple):
    cls: str
    lds: int        # .amdhsa_group_segment_fixed_size
    hwm: int        # slots in use: the highest slot offset / 4, plus one (0: none)
    offsets: tuple  # every ds_write_b32 / ds_read_b32 slot offset, bytes
    solo_marker: bool
    lines: int


_SLOT = re.compile(r"^\s*ds_(?:write|read)_b32 [^\n]*? offset:(\d+)\s*$", re.M)
_DS = re.compile(r"^\s*ds_(?:write|read)_b32 ", re.M)


def facts(src: str) -> Facts:
    """What the emitted text of an eval kernel says about its spills."""
    offs = tuple(int(m) for m in _SLOT.findall(src))
    assert len(offs) == len(_DS.findall(src)), "a ds_write_b32 / ds_read_b32 without a slot offset"
    lds = int(src.split(".amdhsa_group_segment_fixed_size ")[1].split()[0])
    solo = SOLO_MARKER in src
    cls = SOLO if solo else FOUR_WAVE if offs else RESIDENT
    return Facts(cls, lds, max(offs) // 4 + 1 if offs else 0, offs, solo, src.count("\n"))
