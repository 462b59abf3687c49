"""tests/golden/slot_tables.json from a directory of slot-table dumps.

usage: python tests/golden/make_slot_tables.py DUMP_DIR

The dumps are the tables the library uploaded while the layout code still stood in api.hip::rebuild_slots (the commit before
csrc/qp_tables.hpp): that function, patched to write what it is about to upload to the file an environment variable names, run over the
layouts of tests/test_slot_table.py on one MI355X -- a handle per layout and its setters, no kernel.  One file NAME.bin per layout, the
state after the last setter, little-endian:
  int32 magic 0x534c4f54, int32 fit;
  if fit: int32 per_lane, nsoft, total, m_act, n;  int32 kc[n];  double lb[n], ub[n], zw[n], Zw[n];
          if the all-hard table has a 256-lane copy: int32 per_blk;  int32 kc[256 per_blk];  double lb[..], ub[..]
The digest is the one tools/probes/check_slot_table.cpp prints: FNV-1a (64 bit) over the bytes of the eight arrays in that order."""
import json
import os
import struct
import sys


def fnv1a(h, data):
    for byte in data:
        h = ((h ^ byte) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def read(path):
    raw = open(path, "rb").read()
    magic, fit = struct.unpack_from("<ii", raw, 0)
    assert magic == 0x534C4F54, path
    h = 14695981039346656037
    if not fit:
        assert len(raw) == 8, path
        return dict(fit=0, per_lane=0, nsoft=0, total=0, m_act=0, digest=f"{h:016x}")
    per_lane, nsoft, total, m_act, n = struct.unpack_from("<5i", raw, 8)
    assert n == 64 * per_lane, path
    end = 28 + n * (4 + 4 * 8)
    h = fnv1a(h, raw[28:end])
    if len(raw) > end:
        (per_blk,) = struct.unpack_from("<i", raw, end)
        assert per_blk == (n + 255) // 256 and len(raw) == end + 4 + 256 * per_blk * (4 + 2 * 8), path
        h = fnv1a(h, raw[end + 4:])
    return dict(fit=1, per_lane=per_lane, nsoft=nsoft, total=total, m_act=m_act, digest=f"{h:016x}")


def main(dump_dir):
    names = sorted(f[:-4] for f in os.listdir(dump_dir) if f.endswith(".bin"))
    out = {name: read(os.path.join(dump_dir, name + ".bin")) for name in names}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "slot_tables.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(out)} tables -> {path}")


if __name__ == "__main__":
    main(sys.argv[1])
