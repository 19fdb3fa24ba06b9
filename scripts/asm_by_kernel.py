"""Compare two `make asm` outputs of one unit kernel by kernel, for a host-only change that reorders
template instantiations: python scripts/asm_by_kernel.py OLD.s NEW.s

The file is cut at every section directive and at every kernel's entry in the metadata, the pieces
are keyed by the first symbol they name, and the function counter in local labels (.LBB<n>_,
.Lfunc_end<n>), which follows the emission order, is dropped.  Prints each kernel symbol with
"same" or "DIFFERS", then pieces only one file has; exit status 1 unless both files hold the same
pieces with the same text.
"""
import re
import sys


def pieces(path):
    out, cur = {}, []

    def flush():
        if not cur:
            return
        text = re.sub(r"(BB|\.Lfunc_end|\.Lfunc_begin|\.Ltmp)\d+", r"\1", "".join(cur))
        text = re.sub(r"[ \t]+;", " ;", text)  # (comments are padded to a column that the label's width moves)
        m = re.search(r"_Z\w+", text)
        key = (m.group(0) if m else "(no symbol)", cur[0].split()[0])
        out.setdefault(key, []).append(text)

    for line in open(path):
        if re.match(r"\t\.(section|text|rodata|amdgpu_metadata)\b|  - \.(agpr_count|args):|amdhsa\.target:", line):
            flush()
            cur = []
        cur.append(line)
    flush()
    return {k: sorted(v) for k, v in out.items()}


def main():
    a, b = pieces(sys.argv[1]), pieces(sys.argv[2])
    bad = 0
    for sym in sorted({k[0] for k in a} | {k[0] for k in b}):
        ka = {k: v for k, v in a.items() if k[0] == sym}
        kb = {k: v for k, v in b.items() if k[0] == sym}
        same = ka == kb
        bad += not same
        print(f"{'same   ' if same else 'DIFFERS'} {sym} ({sum(len(v) for v in ka.values())} pieces)")
    print(f"{len({k[0] for k in a})} symbols in {sys.argv[1]}, {len({k[0] for k in b})} in {sys.argv[2]}, {bad} differing")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
