"""What every analysis entry point of the library answers before it touches the device: the return code and the text of
``cvx_last_error()`` of a table of calls, compared for equality with ``tests/golden/analysis_refusals.json``.  The fixture pins the
wording of every refusal and, where a call is wrong in more than one way, which fault is reported.

Every call of the table returns BEFORE the entry's first HIP call (decided by reading the entry): it is refused, or it is one of
the accepted cases (k = 0, an empty volume, a ``*_bytes`` query) that return early.  No pointer is dereferenced, so the
addresses are made up, and the test runs without a GPU.  An offset that an entry accepts (4 bytes on a pointer that needs 4-byte
alignment, any offset on a byte volume) would go on to a launch and is therefore not in the table.

The fixture is recorded from the library of the commit BEFORE a change, never from the code under test: copy this module into a
checkout of that commit, build its library there and run

    python tests/test_cpu_refusals.py --record tests/golden/analysis_refusals.json
"""

from __future__ import annotations

import json
import sys
from pathlib import Path

FIXTURE = Path(__file__).resolve().parent / "golden" / "analysis_refusals.json"

INT_MAX, LONG_MAX = 2**31 - 1, 2**63 - 1
BIG = 1 << 40  # a byte count no layout reaches
D0 = (4, 4, 4)  # the extents of a call that is otherwise in order
ERR_HIP = -2


class Ptr:
    """A pointer argument and the alignment its entry asks for (1: none)."""

    def __init__(self, align: int):
        self.align = align


class Entry:
    """One entry point: its arguments in order (``dims`` stands for D, H, W), the values of a call that is in order, whether
    extents above 32768 are refused, and its k argument with the columns of a row where the entry tests that k rows fit."""

    def __init__(self, name, args, *, cap=False, k=None, cols=0, extra=()):
        self.name, self.args, self.cap, self.k, self.cols, self.extra = name, args, cap, k, cols, extra
        self.ptrs = [a for a, v in args if isinstance(v, Ptr)]
        self.has_dims = any(a == "dims" for a, _ in args)

    def good(self) -> dict:
        out = {}
        for i, (a, v) in enumerate(self.args):
            out[a] = (1 << 20) + 4096 * i if isinstance(v, Ptr) else v  # 16-B aligned, every pointer another address
        return out

    def cases(self):
        """Overrides of the good call, one fault (or one early return) each."""
        align = {a: v.align for a, v in self.args if isinstance(v, Ptr)}
        nulls = {p: None for p in self.ptrs}
        if self.has_dims:
            for i in range(3):
                yield {"dims": tuple(-1 if j == i else 4 for j in range(3))}
                wide = {"dims": tuple(32769 if j == i else 4 for j in range(3))}
                # an entry without the cap goes on to its next checks: with every pointer null it is refused there
                yield wide if self.cap or not self.ptrs else {**wide, **nulls}
            yield {"dims": (2048, 1024, 1024)}
            yield {"dims": (INT_MAX, 1, 1)}
            if not self.cap:
                yield {"dims": (1, 2, 4200), **nulls}
                yield {"dims": (1, 1, INT_MAX - 1), **nulls}  # the voxel limit itself
        base = self.good()
        for p in self.ptrs:
            yield {p: None}
            for off in (1, 2, 4, 8):
                if off % align[p] and (off < 8 or align[p] == 16):
                    yield {p: base[p] + off}
        if self.k:
            yield {self.k: -1}
            if self.cols:
                yield {self.k: LONG_MAX // (self.cols * 8) + 1}
                yield {self.k: LONG_MAX}
        yield from self.extra

    def call(self, lib, over: dict):
        vals = {**self.good(), **over}
        flat = []
        for a, _ in self.args:
            flat.extend(vals[a]) if a == "dims" else flat.append(vals[a])
        fn = getattr(lib, self.name)
        if len(flat) < len(fn.argtypes):
            flat.append(None)  # the stream
        return fn(*flat)


P4, P8, P16, P1 = Ptr(4), Ptr(8), Ptr(16), Ptr(1)
EMPTY = {"dims": (0, 4, 4)}

ENTRIES = [
    Entry("cvx_components_scratch_bytes", [("dims", D0)], extra=[EMPTY]),
    Entry("cvx_components_label",
          [("mask", P1), ("dims", D0), ("connectivity", 26), ("min_size", 0), ("labels", P16), ("scratch", P16), ("scratch_bytes", BIG)],
          extra=[{"connectivity": 18}, {"connectivity": 0}, {"min_size": -1}, {"scratch_bytes": 15}, {"scratch_bytes": -1},
                 {"dims": (-1, 4, 4), "connectivity": 18}, {"connectivity": 18, "min_size": -1, "scratch": None}]),
    Entry("cvx_components_table", [("dims", D0), ("k", 1), ("labels", P16), ("table", P8), ("scratch", P16), ("scratch_bytes", BIG)], k="k",
          extra=[{"k": 65}, {"scratch_bytes": 15}, {**EMPTY, "k": 0}, {**EMPTY, "k": 0, "scratch_bytes": 16}, {**EMPTY, "k": 1},
                 {"k": -1, "scratch": None}, {"labels": None, "table": (1 << 20) + 1}]),
    Entry("cvx_edt_squared", [("src", P4), ("src_dtype", 1), ("sites", 0), ("dims", D0), ("out", P4)],
          extra=[{"src_dtype": 2}, {"src_dtype": -1}, {"sites": 2}, {"sites": -1}, EMPTY, {**EMPTY, "src": None, "out": None},
                 {**EMPTY, "src_dtype": 7}, {"dims": (1, 1, 46342)}, {"dims": (1, 1, 46342), "src": None},
                 {"src_dtype": 0, "src": None}, {"src_dtype": 0, "out": (1 << 20) + 2}]),
    Entry("cvx_instance_distance_stats", [("labels", P4), ("d2", P4), ("dims", D0), ("k", 1), ("threshold_d2", 4), ("out", P8)], k="k",
          extra=[{"k": 0}, {"k": 0, "labels": None, "d2": None, "out": None}, {**EMPTY, "k": 0}, {"dims": (-1, 4, 4), "k": -1}]),
    Entry("cvx_instance_shape_stats", [("labels", P4), ("dims", D0), ("k", 1), ("connectivity", 26), ("out", P8)], cap=True, k="k",
          cols=24, extra=[{"connectivity": 18}, {"connectivity": 0}, {"k": 0}, {"k": 0, "labels": None, "out": None},
                          {"k": 0, "connectivity": 18}, {"k": -1, "connectivity": 18}, {**EMPTY, "k": 0},
                          {"dims": (-1, 40000, 4)}, {"dims": (32768, 32768, 2)}, {"dims": (32769, 4, 4), "k": -1}]),
    Entry("cvx_split_core_mask", [("d2", P4), ("dims", D0), ("threshold_d2", 1), ("mask", P1)],
          extra=[{"threshold_d2": -1}, EMPTY, {**EMPTY, "d2": None, "mask": None}, {**EMPTY, "threshold_d2": -1}]),
    Entry("cvx_split_init", [("labels", P4), ("cores", P4), ("dims", D0), ("k", 1), ("m", 1), ("has_core", P4), ("keys", P8)], k="k",
          extra=[{"m": -1}, {"k": 65}, {"m": 65}, {**EMPTY, "k": 0, "m": 0}, {**EMPTY, "k": 1, "m": 0},
                 {**EMPTY, "k": 0, "m": 0, "labels": None, "keys": None}]),
    Entry("cvx_split_rounds", [("labels", P4), ("keys", P8), ("dims", D0), ("connectivity", 26), ("rounds", 1), ("changed", P4)],
          extra=[{"connectivity": 18}, {"rounds": 0}, {"rounds": -1}, {"connectivity": 18, "rounds": 0}, {**EMPTY, "changed": None}]),
    Entry("cvx_split_first", [("labels", P4), ("keys", P8), ("dims", D0), ("seeds", 2), ("first", P4)],
          extra=[{"seeds": -1}, {"seeds": 129}, {**EMPTY, "seeds": 1}, {**EMPTY, "seeds": 0, "first": None}]),
    Entry("cvx_split_relabel",
          [("labels", P4), ("keys", P8), ("rank", P4), ("dims", D0), ("seeds", 2), ("kp", 1), ("labels_out", P4), ("table", P8),
           ("component", P8)],
          extra=[{"seeds": -1}, {"seeds": 129}, {"kp": -1}, {"kp": 3}, {**EMPTY, "seeds": 0, "kp": 0},
                 {**EMPTY, "seeds": 0, "kp": 0, "labels": None}, {**EMPTY, "seeds": 1, "kp": 0}]),
    Entry("cvx_nearest_workspace_bytes", [("dims", D0)], extra=[EMPTY]),
    Entry("cvx_nearest_instance", [("labels", P4), ("k", 1), ("dims", D0), ("d2_out", P4), ("nearest_out", P4), ("workspace", P8)], k="k",
          extra=[EMPTY, {**EMPTY, "labels": None, "workspace": None}, {**EMPTY, "k": -1}, {"dims": (1, 1, 46342)},
                 {"dims": (1, 1, 46342), "labels": None}]),
    Entry("cvx_instance_pair_contacts",
          [("labels_a", P4), ("ka", 1), ("nearest_b", P4), ("d2_b", P4), ("threshold_d2", 4), ("dims", D0), ("table", P8),
           ("capacity", 64), ("status", P8)], k="ka",
          extra=[{"capacity": 0}, {"capacity": -1}, {"capacity": 3}, {"capacity": 2**32}, {"capacity": 2**31, "table": None},
                 {"ka": -1, "capacity": 3}, {**EMPTY, "capacity": 3}]),
    Entry("cvx_instance_pair_rows", [("table", P8), ("capacity", 64), ("order", P8), ("p", 1), ("rows", P8)],
          extra=[{"capacity": 0}, {"capacity": 3}, {"capacity": 2**32}, {"p": -1}, {"p": 65}, {"p": 0},
                 {"p": 0, "table": None, "order": None, "rows": None}, {"capacity": 3, "p": -1}]),
    Entry("cvx_skeleton_init", [("labels", P4), ("dims", D0), ("k", 1), ("alive", P4)], cap=True, k="k",
          extra=[EMPTY, {**EMPTY, "labels": None, "alive": None}, {**EMPTY, "k": -1}, {"dims": (32769, 4, 4), "k": -1},
                 {"dims": (32768, 32768, 2)}]),
    Entry("cvx_skeleton_cycles",
          [("alive", P4), ("d2", P4), ("dims", D0), ("k", 1), ("level_d2", 4), ("end_d2", 4), ("cycles", 1), ("changed", P4)],
          cap=True, k="k", extra=[{"end_d2": 0}, {"level_d2": -1}, {"cycles": 0}, {"end_d2": 0, "level_d2": -1, "cycles": 0},
                                  {"level_d2": -1, "cycles": 0}, {"k": -1, "end_d2": 0}, {**EMPTY, "changed": None},
                                  {"dims": (32768, 32768, 2)}]),
    Entry("cvx_skeleton_stats", [("alive", P4), ("d2", P4), ("dims", D0), ("k", 1), ("table", P8)], cap=True, k="k", cols=8,
          extra=[{"k": 0}, {"k": 0, "alive": None, "d2": None, "table": None}, {**EMPTY, "k": 0}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_local_thickness_workspace_bytes", [("dims", D0)], cap=True,
          extra=[EMPTY, {"dims": (5, 9, 65)}, {"dims": (32768, 32768, 1)}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_local_thickness_squared", [("d2", P4), ("dims", D0), ("t2", P4), ("workspace", P4), ("workspace_bytes", BIG)], cap=True,
          extra=[EMPTY, {**EMPTY, "d2": None, "t2": None, "workspace": None}, {"workspace_bytes": 7}, {"workspace_bytes": -1},
                 {"t2": 1 << 20}, {"t2": 1 << 20, "workspace_bytes": 7}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_instance_thickness_stats", [("labels", P4), ("t2", P4), ("dims", D0), ("k", 1), ("table", P8)], cap=True, k="k", cols=5,
          extra=[{"k": 0}, {"k": 0, "labels": None, "t2": None, "table": None}, {**EMPTY, "k": 0},
                 {"k": INT_MAX * 256 // 5 + 64}, {"k": INT_MAX * 256 // 5 + 64, "table": None}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_mesh_workspace_bytes", [("dims", D0)], cap=True,
          extra=[EMPTY, {"dims": (5, 9, 65)}, {"dims": (32768, 32768, 1)}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_mesh_count", [("labels", P4), ("dims", D0), ("workspace", P16), ("workspace_bytes", BIG), ("totals", P8)], cap=True,
          extra=[{"workspace_bytes": 15}, {"workspace_bytes": -1}, {**EMPTY, "workspace_bytes": 15}, {**EMPTY, "totals": None},
                 {"dims": (32768, 32768, 2)}]),
    Entry("cvx_mesh_emit",
          [("labels", P4), ("dims", D0), ("workspace", P16), ("workspace_bytes", BIG), ("V", 3), ("T", 3), ("vertices", P4),
           ("triangles", P4), ("ids", P4)], cap=True,
          extra=[{"V": -1}, {"T": -1}, {"V": 2**31}, {"T": 2**31}, {"V": -1, "T": 2**31}, {"workspace_bytes": 15},
                 {"V": 0, "T": 0}, {"V": 0, "T": 0, "vertices": None, "triangles": None, "ids": None}, {"V": 0, "T": 0, "workspace_bytes": 15},
                 {"V": 0, "vertices": None, "workspace_bytes": 15}, {**EMPTY, "V": 0, "T": 0}, {**EMPTY, "V": 3, "T": 0}, {**EMPTY, "V": 0, "T": 3},
                 {**EMPTY, "V": 0, "T": 0, "workspace_bytes": 15}, {**EMPTY, "V": 0, "T": 0, "labels": None},
                 {"dims": (32768, 32768, 2)}]),
    Entry("cvx_mesh_stats", [("vertices", P4), ("triangles", P4), ("ids", P4), ("V", 3), ("T", 3), ("k", 1), ("table", P8)], k="k", cols=3,
          extra=[{"V": -1}, {"T": -1}, {"V": 2**31}, {"T": 2**31}, {"k": 0}, {"k": 0, "ids": None, "table": None},
                 {"k": 0, "vertices": None}, {"k": -1, "V": -1}, {"V": 0, "vertices": None, "k": 0}]),
    Entry("cvx_mesh_smooth_workspace_bytes", [("V", 3)], extra=[{"V": 0}, {"V": -1}, {"V": 2**31 - 1}, {"V": 2**31}]),
    Entry("cvx_mesh_smooth_step",
          [("vertices", P4), ("moved", P4), ("triangles", P4), ("V", 3), ("T", 3), ("c", 32768), ("workspace", P8), ("workspace_bytes", BIG)],
          extra=[{"V": -1}, {"T": -1}, {"V": 2**31}, {"c": 131073}, {"c": -131073}, {"workspace_bytes": 95}, {"workspace_bytes": -1},
                 {"V": 0, "T": 0}, {"V": 0, "T": 0, "vertices": None, "moved": None, "triangles": None, "workspace": None},
                 {"V": 0, "c": 131073}, {"c": 131073, "moved": None}]),
    Entry("cvx_mask_flood_pack", [("mask", P1), ("dims", D0), ("slices", 0), ("open", P8), ("reach", P8)],
          extra=[{"slices": 2}, {"slices": -1}, {"slices": 2, "open": None}, EMPTY, {**EMPTY, "mask": None, "open": None, "reach": None},
                 {**EMPTY, "slices": 2}, {"reach": (1 << 20) + 4096 * 3}]),  # reach = open
    Entry("cvx_mask_flood_rounds",
          [("open", P8), ("reach", P8), ("dims", D0), ("background", 6), ("slices", 0), ("rounds", 1), ("changed", P4)],
          extra=[{"background": 18}, {"background": 0}, {"slices": 2}, {"rounds": 0}, {"rounds": -1}, {"background": 18, "rounds": 0},
                 {"slices": 2, "changed": None}, EMPTY, {**EMPTY, "open": None, "reach": None}, {**EMPTY, "changed": None},
                 {"reach": 1 << 20}]),  # reach = open
    Entry("cvx_mask_flood_unpack", [("reach", P8), ("dims", D0), ("out", P1)], extra=[EMPTY, {**EMPTY, "reach": None, "out": None}]),
    Entry("cvx_mask_threshold", [("d2", P4), ("dims", D0), ("pad", 1), ("mode", 0), ("threshold_d2", 4), ("out", P1)],
          extra=[{"pad": -1}, {"pad": 32769}, {"pad": 32768}, {"dims": (1, 1, INT_MAX - 1), "pad": 1}, {"mode": 2}, {"mode": -1},
                 {"threshold_d2": -1}, {"threshold_d2": INT_MAX}, {"mode": 2, "threshold_d2": -1}, {"pad": -1, "mode": 2}, EMPTY,
                 {**EMPTY, "d2": None, "out": None}, {**EMPTY, "mode": 2}]),
    Entry("cvx_mask_added_voxels", [("labels", P4), ("before", P1), ("dims", D0), ("k", 1), ("out", P8)], k="k", cols=1,
          extra=[{"k": 0}, {"k": 0, "labels": None, "before": None, "out": None}, {**EMPTY, "k": 0}, {"dims": (-1, 4, 4), "k": -1}]),
    Entry("cvx_curvature_workspace_bytes", [("dims", D0)], cap=True,
          extra=[EMPTY, {"dims": (5, 9, 65)}, {"dims": (5, 9, 64)}, {"dims": (32768, 32768, 1)}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_curvature_map", [("labels", P4), ("dims", D0), ("radius", 2), ("h", P4), ("workspace", P8), ("workspace_bytes", BIG)], cap=True,
          extra=[{"radius": 1}, {"radius": 17}, {"radius": 1, "labels": None}, {"dims": (32769, 4, 4), "radius": 1}, EMPTY,
                 {**EMPTY, "labels": None, "h": None, "workspace": None}, {**EMPTY, "radius": 1}, {"workspace_bytes": 127},
                 {"workspace_bytes": -1}, {"h": 1 << 20}, {"h": 1 << 20, "workspace_bytes": 127}, {"dims": (32768, 32768, 2)}]),  # h = labels
    Entry("cvx_curvature_stats", [("labels", P4), ("h", P4), ("dims", D0), ("k", 1), ("table", P8)], cap=True, k="k", cols=7,
          extra=[{"k": 0}, {"k": 0, "labels": None, "h": None, "table": None}, {**EMPTY, "k": 0},
                 {"k": INT_MAX * 256 // 7 + 64}, {"k": INT_MAX * 256 // 7 + 64, "table": None}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_pick_workspace_bytes", [("dims", D0)], cap=True,
          extra=[EMPTY, {"dims": (5, 9, 65)}, {"dims": (5, 9, 64)}, {"dims": (32768, 32768, 1)}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_pick_pack",
          [("labels", P4), ("dims", D0), ("k", 1), ("radius", 2), ("fg", P8), ("state", P8), ("workspace_bytes", BIG)], cap=True, k="k",
          extra=[{"radius": 1}, {"radius": 17}, {"radius": 1, "k": -1}, {"k": 0}, {"k": 0, "labels": None, "fg": None, "state": None},
                 {"k": 0, "radius": 1}, EMPTY, {**EMPTY, "k": -1}, {"workspace_bytes": 127}, {"workspace_bytes": -1},
                 {"state": (1 << 20) + 4096 * 4}, {"fg": (1 << 20) + 4096 * 5 + 128},  # state = fg; fg = state[1]
                 {"dims": (32768, 32768, 2)}]),
    Entry("cvx_pick_rounds",
          [("labels", P4), ("dims", D0), ("k", 1), ("spacing", 2), ("seed", 0), ("rounds", 1), ("state_a", P8), ("state_b", P8),
           ("workspace_bytes", BIG), ("changed", P4)], cap=True, k="k",
          extra=[{"spacing": 1}, {"spacing": 17}, {"rounds": 0}, {"rounds": -1}, {"spacing": 1, "rounds": 0}, {"rounds": 0, "changed": None},
                 {"k": 0, "changed": None}, {**EMPTY, "changed": None}, {"workspace_bytes": 127}, {"workspace_bytes": -1},
                 {"state_b": (1 << 20) + 4096 * 6 + 8}, {"state_b": (1 << 20) + 4096 * 6 + 248},  # inside state_a's two bitmaps
                 {"state_a": (1 << 20) + 4096 * 7 + 248}, {"dims": (32768, 32768, 2)}]),
    Entry("cvx_pick_count", [("state", P8), ("dims", D0), ("workspace_bytes", BIG), ("row_first", P4), ("total", P8)], cap=True,
          extra=[{"workspace_bytes": 127}, {"workspace_bytes": -1}, {**EMPTY, "total": None}, {**EMPTY, "total": (1 << 20) + 4},
                 {"dims": (32768, 32768, 2)}]),
    Entry("cvx_pick_emit",
          [("labels", P4), ("fg", P8), ("state", P8), ("row_first", P4), ("dims", D0), ("radius", 2), ("workspace_bytes", BIG), ("P", 1),
           ("table", P4)], cap=True,
          extra=[{"radius": 1}, {"radius": 17}, {"P": -1}, {"P": 65}, {"radius": 1, "P": -1}, {"P": 0},
                 {"P": 0, "labels": None, "fg": None, "state": None, "row_first": None, "table": None}, {"P": 0, "workspace_bytes": 127},
                 {"workspace_bytes": 127}, {"workspace_bytes": -1}, {**EMPTY, "P": 0}, {**EMPTY, "P": 1}, {"dims": (32768, 32768, 2)}]),
]


def case_id(entry: Entry, over: dict) -> str:
    return entry.name + "(" + ", ".join(f"{a}={over[a]}" for a, _ in entry.args if a in over) + ")"


def table():
    seen = {}
    for e in ENTRIES:
        for over in e.cases():
            seen.setdefault(case_id(e, over), (e, over))  # a fault listed twice is one call
    return seen


def run(lib) -> dict:
    """id -> [return code, cvx_last_error() after the call].  The text is reset to a known one before every call, so that a call
    which records none (a success, a ``*_bytes`` query) shows that too."""
    out = {}
    for cid, (e, over) in table().items():
        assert lib.cvx_device_arch(None, 0) == -1  # refused on its first line: "cvx_device_arch: bad buffer"
        rc = e.call(lib, over)
        out[cid] = [int(rc), lib.cvx_last_error().decode()]
    return out


def load_lib():
    from cryovit_amd import _lib
    from cryovit_amd.build import build_library

    build_library()
    return _lib.load()


def test_table_covers_every_analysis_entry():
    from cryovit_amd import _lib

    prefixes = ("cvx_components_", "cvx_edt_", "cvx_instance_", "cvx_split_", "cvx_nearest_", "cvx_skeleton_", "cvx_local_thickness_",
                "cvx_mesh_", "cvx_mask_", "cvx_curvature_", "cvx_pick_")
    want = {n for n in _lib.SIGNATURES if n.startswith(prefixes)} - {"cvx_split_stream"}  # the encoder's, no analysis entry
    assert want == {e.name for e in ENTRIES}
    for e in ENTRIES:
        n = sum(3 if a == "dims" else 1 for a, _ in e.args)
        assert n in (len(_lib.SIGNATURES[e.name][1]), len(_lib.SIGNATURES[e.name][1]) - 1), e.name  # with or without a stream


def test_refusals_equal_the_recorded_ones():
    want = json.loads(FIXTURE.read_text())
    assert not [c for c, (rc, _) in want.items() if rc == ERR_HIP], "a recorded call reached the device"
    got = run(load_lib())
    assert sorted(got) == sorted(want)  # the table and the fixture list the same calls
    wrong = {c: (got[c], want[c]) for c in want if got[c] != want[c]}
    assert not wrong, wrong


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "--record":
        sys.exit(__doc__)
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
    recorded = run(load_lib())
    reached = [c for c, (rc, _) in recorded.items() if rc == ERR_HIP]
    assert not reached, f"these calls reached the device and do not belong in the table: {reached}"
    lines = ",\n".join(f"{json.dumps(c)}: {json.dumps(recorded[c])}" for c in sorted(recorded))  # one call per line
    Path(sys.argv[2]).write_text("{\n" + lines + "\n}\n")
    print(f"{len(recorded)} calls recorded")
