"""The table-driven status grid behind tests/wino_status_cases.py and tests/conv_status_cases.py: for every listed entry point one valid
call on a small geometry (made-up pointer values, as in tests/test_host_cpu.py) and that call with every single defect and every pair
of defects from a fixed list.  Every tuple is one the library must refuse before it enqueues anything; the status it returns -- which
of several applicable ones wins included -- is recorded in a fixture under tests/golden/ (`python tests/<cases file> --record`, run
against the library the statuses are to be held to, on a machine without a GPU).

An entry's arguments are listed in the order of its C signature, each as (name, kind[, value]):
  P  required f32 pointer, 16-byte aligned          p  optional one (given in the valid call)      n  optional, not given
  R  required pointer whose alignment is not checked
  B / b  required / optional 64-bit mask words (8-byte aligned)          a  optional argmax bytes (4-byte aligned), A required
  G  the geometry (NULL is a defect too), H the geometry of the layer below (ssd_wino4_adj_output_to_planes)
  W  the workspace pointer, Z<x> its size: the value the cases file's size query returns under that name
  i  an int (value given), u a pointer or int no rule looks at (passed as given), S the stream (NULL)

A defect is (label, {argument or "g.<name>": value}); "g.<name>" is an argument of ops.make_geom or, where make_geom has none of that
name, a field of the geometry, set after make_geom has derived Ho and Wo.
"""
import itertools
import json
import os

OK_PTR, ODD_PTR, ODD_BYTES = 0x10000, 0x10004, 0x10002
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


class Grid:
    """entries: {entry: [(name, kind[, value])]}; extra: {entry: [defect]} beyond those the argument kinds imply (a NULL for every
    required pointer and the geometry, a misaligned value for every pointer with an alignment rule, a workspace one byte short);
    geom: ops.make_geom arguments of the valid call, geom_of: {entry: those of an entry that needs another map};
    sizes: (lib, make_geom, byref) -> {"Z<x>": bytes} of the valid geometry; valid_launches: the recorder also holds every entry's
    defect-free call to SSD_ERR_LAUNCH, the answer of an accepted call on a machine without a GPU."""

    def __init__(self, fixture, entries, extra, geom, sizes, geom_of=None, valid_launches=False):
        assert set(extra) == set(entries)
        self.fixture, self.entries, self.extra, self.geom, self.sizes = os.path.join(GOLDEN, fixture), entries, extra, geom, sizes
        self.geom_of, self.valid_launches = geom_of or {}, valid_launches

    def defects(self, entry):
        """Every defect of one entry, in a fixed order: those its argument kinds imply, then extra[entry]."""
        out = []
        for name, kind, *_ in self.entries[entry]:
            if kind in "PRBAWGH":
                out.append((f"null:{name}", {name: None}))
            if kind in "PpnBbW":
                out.append((f"odd:{name}", {name: ODD_PTR}))
            if kind in "Aa":
                out.append((f"odd:{name}", {name: ODD_BYTES}))
            if kind.startswith("Z"):
                out.append(("ws-1", {name: -1}))                 # relative to the queried size
        return out + self.extra[entry]

    def cases(self, entry):
        """[(label, {argument: value})]: every single defect and every pair that does not set one argument twice"""
        d = self.defects(entry)
        out = [(la, dict(ch)) for la, ch in d]
        for (la, ca), (lb, cb) in itertools.combinations(d, 2):
            if not set(ca) & set(cb):
                out.append((f"{la}+{lb}", {**ca, **cb}))
        return out

    def arguments(self, entry, changes, sizes, make_geom, byref):
        """The ctypes arguments of `entry` for the valid call (`changes` empty) or a defective one.  sizes: as the size query returns
        them; make_geom: ops.make_geom; byref: ctypes.byref.  The geometries are returned too: they must outlive the call."""
        base = self.geom_of.get(entry, self.geom)
        of_g = {k[2:]: v for k, v in changes.items() if k.startswith("g.")}
        g = make_geom(**dict(base, **{k: v for k, v in of_g.items() if k in base}))
        for k, v in of_g.items():
            if k not in base:
                setattr(g, k, v)
        below = make_geom(**dict(base, co=base["ci"]))
        args = []
        for name, kind, *value in self.entries[entry]:
            if name in changes and not kind.startswith("Z"):
                v = changes[name]
                args.append(v if kind not in "GH" else None)
            elif kind in "PpRBbAW":
                args.append(OK_PTR)
            elif kind in "naS":
                args.append(None)
            elif kind == "G":
                args.append(byref(g))
            elif kind == "H":
                args.append(byref(below))
            elif kind.startswith("Z"):
                args.append(sizes[kind] + changes.get(name, 0))
            else:
                args.append(value[0])
        return args, (g, below)

    def statuses(self, lib, make_geom, byref, valid=False):
        """{entry: {label: status}} of the loaded library, over every case (valid: over the defect-free call alone, as {entry: status})"""
        sizes = self.sizes(lib, make_geom, byref)
        assert all(v > 0 for v in sizes.values()), sizes
        out = {}
        for entry in self.entries:
            fn = getattr(lib, entry)
            out[entry] = {}
            for label, changes in [("", {})] if valid else self.cases(entry):
                args, keep = self.arguments(entry, changes, sizes, make_geom, byref)
                out[entry][label] = fn(*args)
        return {e: d[""] for e, d in out.items()} if valid else out

    def record(self):
        """Write the fixture from the importable library.  Refuses where a GPU is present (a tuple the library accepted would be
        launched on made-up pointers) and where the library accepts any tuple: 0, or SSD_ERR_LAUNCH (-4) from the launch that fails
        without a GPU."""
        import ctypes
        import sys
        import torch
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from objectdetection_ssd_amd import _lib, ops
        if torch.cuda.is_available():
            raise SystemExit("record on a machine without a GPU")
        if self.valid_launches:
            unsound = {e: s for e, s in self.statuses(_lib.load(), ops.make_geom, ctypes.byref, valid=True).items() if s != -4}
            if unsound:
                raise SystemExit(f"the defect-free call does not reach its launch: {unsound}")
        got = self.statuses(_lib.load(), ops.make_geom, ctypes.byref)
        accepted = [(e, la, s) for e, d in got.items() for la, s in d.items() if s in (0, -4)]
        if accepted:
            raise SystemExit("accepted, so no defect of that entry:\n" + "\n".join(f"  {e} {la}: {s}" for e, la, s in accepted))
        with open(self.fixture, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True)
            f.write("\n")
        print(f"{sum(len(d) for d in got.values())} cases of {len(got)} entries -> {self.fixture}")
