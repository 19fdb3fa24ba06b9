#!/usr/bin/env python3
"""Do two trees' scene compilers (eraytracer_amd/csrc/rt_scene.cpp) produce the same bytes?

    python scripts/scene_compile_diff.py PARENT_CSRC HEAD_CSRC [--asm PARENT_ASM HEAD_ASM]
        [--mutant NAME=CSRC ...] [--ab PAIRS]

PARENT_CSRC and HEAD_CSRC are the eraytracer_amd/csrc directories of two checkouts (for the parent:
`git worktree add DIR HEAD~` and DIR/eraytracer_amd/csrc; the headers are found from there).  The dump
program of the head tree (tests/csrc/scene_dump.cpp) is built against each, twice — g++ -O1 with the
host sanitizers, and hipcc -x c++ with the Makefile's CXXFLAGS, the host compiler that ships — and
run over tests/scene_corpus.py under two environments: none, and the three knobs set.  Per scene the
two sides' dumps are compared section by section.  The result goes to
profiles/scene_compile_equiv.txt; the exit status is 0 only if every scene was dumped by both sides
with the expected return code, at least one byte was compared everywhere, and no byte differs.

--asm: two directories holding `make asm`'s output for the two trees; the files are compared too.
--mutant: a csrc directory that is meant to differ (the comparison's own check); which scenes differ
  from the parent is recorded, and the status is 1 if none does.
--ab PAIRS: alternate the two hipcc builds PAIRS times over three scenes and write compile_scene's
  host milliseconds to profiles/scene_compile_ab.txt.
"""
import argparse
import filecmp
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import scene_corpus  # noqa: E402

DUMP = os.path.join(ROOT, "tests", "csrc", "scene_dump.cpp")
KNOBS = {"RT_BVH_MIN": "2", "RT_BVH_LEVEL": "1", "RT_BEAM_MIN": "1"}
ENVS = {"default": {}, "knobs": KNOBS}
ASAN = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
        "-fno-sanitize-recover=all"]
AB_SCENES = ("s256", "synthetic2048", "synthetic5000")


def makefile_cxxflags(csrc):
    with open(os.path.join(csrc, "Makefile")) as f:
        return re.search(r"^CXXFLAGS := (.*)$", f.read(), re.M).group(1).split()


def build(csrc, kind, out):
    if kind == "asan":
        cmd = ASAN
    else:
        cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "c++"] + makefile_cxxflags(csrc)
    subprocess.run(cmd + ["-I", csrc, DUMP, os.path.join(csrc, "rt_scene.cpp"), "-o", out], check=True)
    return out


def run(exe, env_extra, outdir, files):
    """Dumps of `files` into outdir; returns {file's base name: compile_scene's milliseconds}."""
    os.makedirs(outdir, exist_ok=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("RT_")}
    env.update(env_extra)
    r = subprocess.run([exe, outdir] + files, capture_output=True, text=True, env=env)
    if r.returncode != 0:
        raise SystemExit(f"{exe} failed ({r.returncode}):\n{r.stderr}")
    return {ln.split()[0]: float(ln.split()[1]) for ln in r.stdout.splitlines()}


def sections(path):
    """A dump as {section name: bytes}."""
    with open(path, "rb") as f:
        data = f.read()
    out, at = {}, 0
    while at < len(data):
        nl = data.index(b"\n", at)
        name, size = data[at:nl].split()
        out[name.decode()] = data[nl + 1:nl + 1 + int(size)]
        at = nl + 1 + int(size)
    return out


def compare(names, dir_a, dir_b, problems, where):
    """Bytes compared, and the scenes that differ (with the sections) appended to `problems`."""
    total, differing = 0, []
    for i, name in enumerate(names):
        pa, pb = (os.path.join(d, f"{i:03d}.bin.dump") for d in (dir_a, dir_b))
        if not (os.path.exists(pa) and os.path.exists(pb)):
            problems.append(f"{where}: {name}: missing on one side")
            continue
        a, b = sections(pa), sections(pb)
        want = scene_corpus.BAD.get(name, 0)
        for side, s in (("first", a), ("second", b)):
            rc = int.from_bytes(s["rc"][8:12], "little", signed=True)
            if rc != want:
                problems.append(f"{where}: {name}: compile_scene returned {rc} on the {side} side, expected {want}")
        bad = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        if bad:
            differing.append(name)
            problems.append(f"{where}: {name}: differs in {', '.join(bad)}")
        total += sum(len(v) for v in a.values())
    return total, differing


def ab(exes, files_by_name, pairs, path):
    rows = {name: {"parent": [], "head": []} for name in AB_SCENES}
    with tempfile.TemporaryDirectory() as tmp:
        for _ in range(pairs):
            for side in ("parent", "head"):
                for name in AB_SCENES:
                    ms = run(exes[side], {}, tmp, [files_by_name[name]])
                    rows[name][side].append(next(iter(ms.values())))
    ok = True
    with open(path, "w") as f:
        f.write(f"compile_scene, host wall-clock ms, hipcc -O3 host build of tests/csrc/scene_dump.cpp; {pairs} alternated "
                "pairs (parent, head) per scene.\nRule: every head run within the parent's range widened by its own width, "
                "or faster.\n\n")
        for name, r in rows.items():
            lo, hi = min(r["parent"]), max(r["parent"])
            limit = hi + (hi - lo)
            good = all(v <= limit for v in r["head"])
            ok = ok and good
            f.write(f"{name}\n  parent {' '.join(f'{v:.2f}' for v in r['parent'])}\n"
                    f"  head   {' '.join(f'{v:.2f}' for v in r['head'])}\n"
                    f"  parent range [{lo:.2f}, {hi:.2f}], limit {limit:.2f}, head max {max(r['head']):.2f}: "
                    f"{'within' if good else 'SLOWER'}\n")
    return ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent_csrc")
    ap.add_argument("head_csrc")
    ap.add_argument("--asm", nargs=2, metavar=("PARENT_ASM", "HEAD_ASM"))
    ap.add_argument("--mutant", action="append", default=[], metavar="NAME=CSRC")
    ap.add_argument("--ab", type=int, default=0, metavar="PAIRS")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scene_compile_equiv.txt"))
    a = ap.parse_args()
    corpus = scene_corpus.corpus()
    names = list(corpus)
    lines, problems = [], []
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for i, name in enumerate(names):
            files.append(os.path.join(tmp, f"{i:03d}.bin"))
            with open(files[-1], "wb") as f:
                f.write(scene_corpus.records(corpus[name]))
        exes = {}
        for kind in ("asan", "hipcc"):
            for side, csrc in (("parent", a.parent_csrc), ("head", a.head_csrc)):
                exes[kind, side] = build(os.path.abspath(csrc), kind, os.path.join(tmp, f"dump_{side}_{kind}"))
            for env_name, env in ENVS.items():
                dirs = {side: os.path.join(tmp, f"{side}_{kind}_{env_name}") for side in ("parent", "head")}
                for side in dirs:
                    run(exes[kind, side], env, dirs[side], files)
                where = f"{kind} build, {env_name} environment"
                total, differing = compare(names, dirs["parent"], dirs["head"], problems, where)
                if total == 0:
                    problems.append(f"{where}: nothing was compared")
                lines.append(f"{where}: {len(names)} scenes, {total} bytes compared, {len(differing)} scenes differ")
        # the two builds agree with each other too (head, default environment)
        total, differing = compare(names, os.path.join(tmp, "head_asan_default"), os.path.join(tmp, "head_hipcc_default"),
                                   problems, "head: asan against hipcc build")
        lines.append(f"head, sanitized g++ -O1 against hipcc -O3: {total} bytes compared, {len(differing)} scenes differ")
        for spec in a.mutant:
            label, csrc = spec.split("=", 1)
            exe = build(os.path.abspath(csrc), "hipcc", os.path.join(tmp, f"dump_mutant_{label}"))
            out = os.path.join(tmp, f"mutant_{label}")
            run(exe, {}, out, files)
            found = []
            _, differing = compare(names, os.path.join(tmp, "parent_hipcc_default"), out, found, label)
            lit = [n for n in names if n not in scene_corpus.BAD and
                   {"sphere", "point_light"} <= {t[0] for t in corpus[n]}]
            same = [n for n in lit if n not in differing]
            lines.append(f"mutant {label} (hipcc build, default environment): {len(differing)} of {len(names)} scenes "
                         f"differ{' (' + ', '.join(differing) + ')' if len(differing) <= 10 else ''}; of the {len(lit)} "
                         f"compiling scenes with a sphere and a light {len(same)} are unchanged")
            if not differing:
                problems.append(f"mutant {label}: no scene differs")
        if a.asm:
            units = sorted(f for f in os.listdir(a.asm[0]) if f.endswith(".s"))
            same = [u for u in units if os.path.exists(os.path.join(a.asm[1], u)) and
                    filecmp.cmp(os.path.join(a.asm[0], u), os.path.join(a.asm[1], u), shallow=False)]
            lines.append(f"make asm, parent against head: {len(same)} of {len(units)} files byte-identical "
                         f"({', '.join(units)})")
            if not units or same != units:
                problems.append("make asm: the device code differs: " + ", ".join(sorted(set(units) - set(same))))
        if a.ab:
            ab_ok = ab({"parent": exes["hipcc", "parent"], "head": exes["hipcc", "head"]}, dict(zip(names, files)), a.ab,
                       os.path.join(os.path.dirname(a.out), "scene_compile_ab.txt"))
            if not ab_ok:
                problems.append("compile time: a head run is outside the rule (see scene_compile_ab.txt)")
    with open(a.out, "w") as f:
        f.write("Scene compiler, parent against head: every byte of check / canon / compile codes, SceneHdr, tab, itab,\n"
                "elem_of and canon_of per scene of tests/scene_corpus.py (scripts/scene_compile_diff.py).\n"
                f"knobs environment: {' '.join(f'{k}={v}' for k, v in KNOBS.items())}\n\n")
        f.write("\n".join(lines) + "\n\n")
        f.write("\n".join(problems) + "\n" if problems else "no difference, nothing missing\n")
    print(open(a.out).read())
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main())
