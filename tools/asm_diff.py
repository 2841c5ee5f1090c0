#!/usr/bin/env python3
"""Compare two compiler outputs kernel by kernel:  tools/asm_diff.py PARENT_DIR NEW_DIR [--md] [--not-worse]

Both directories hold the gfx950 assembly of the same sources (hipcc FLAGS --cuda-device-only -S X.hip -o DIR/X.s, FLAGS as
in fullsubnet_plus_amd/_build.py).  Per kernel symbol the verdict is
  identical  the function's text and its metadata are equal (the `.file` lines and the function number in local labels aside), or
  (ii)       equal register / spill / scratch / LDS / kernarg figures, opcode-for-opcode equal depth-2 loops that hold an MFMA,
             a time loop (the depth-1 loop with the most MFMAs) that is not longer and holds the same number of MFMAs, 16-byte
             buffer loads, LDS reads, LDS writes, barriers and waits; a kernel WITHOUT a depth-2 MFMA loop (a GEMM: its k-loop is
             the depth-1 loop) must keep that time loop opcode for opcode instead, or
  DIFFERENT  with the figures that differ.
With --not-worse a kernel WITHOUT a depth-2 MFMA loop on either side (the column-split recurrent kernels: their k-loops are unrolled
into a time loop of thousands of instructions, which a freed register reorders) that would be DIFFERENT is instead
  (iii)      "not worse": no register / spill / scratch figure higher, LDS and kernarg equal, a time loop that is not longer and holds
             the same number of MFMAs and 16-byte buffer loads and no more LDS reads, LDS writes, barriers or waits.
Exit status 1 if any kernel is DIFFERENT or missing on one side."""
import os
import re
import sys

META = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size", ".kernarg_segment_size")
COUNTED = (r"v_mfma", r"buffer_load_dwordx4", r"ds_read", r"ds_write", r"s_barrier", r"s_waitcnt")


def instructions(lines):
    out = []
    for l in lines:
        s = l.split(";")[0].strip()
        if s and not s.startswith(".") and not s.endswith(":"):
            out.append(s)
    return out


BLOCK = re.compile(r"^(?:(\.LBB\d+_\d+):|; %bb\.\d+:)")


def loops(body, depth):
    """[(first line, last line)] of every loop of the given depth, from the compiler's loop comments.  Depth 2 (single-block k-group
    loops): header to its backward branch.  Depth 1: the span of the blocks the compiler marks as part of the loop (the header need
    not come first in the layout)."""
    res = []
    starts = [i for i, l in enumerate(body) if BLOCK.match(l)] + [len(body)]
    for i, l in enumerate(body):
        if f"Loop Header: Depth={depth}" not in l:
            continue
        lab = next((m.group(1) for k in range(i, max(i - 4, -1), -1) for m in [re.match(r"^(\.LBB\d+_\d+):", body[k])] if m), None)
        if lab is None:
            continue
        if depth == 2:
            back = [k for k in range(i, len(body)) if re.search(r"s_cbranch_\w+ " + re.escape(lab) + r"\b", body[k])]
            if back:
                res.append((i, back[0]))
            continue
        mark = re.compile(r"(Header=|Parent Loop )" + re.escape(lab[2:]) + r"\b")
        mine = [k for k in range(len(starts) - 1) if starts[k] <= i < starts[k + 1] or any(mark.search(x) for x in body[starts[k]:starts[k] + 3])]
        res.append((starts[mine[0]], starts[mine[-1] + 1] - 1))
    return res


def kernels(path):
    text = "\n".join(l for l in open(path).read().split("\n") if not l.lstrip().startswith(".file"))
    meta = {}
    for entry in re.split(r"^  - (?=\.)", text[text.find("amdhsa.kernels:"):], flags=re.M)[1:]:
        entry = "    " + entry
        name = re.search(r"^    \.name:\s+(\S+)", entry, re.M)
        if name:
            meta[name.group(1)] = {k: re.search(r"^    " + re.escape(k) + r":\s+(\S+)", entry, re.M).group(1) for k in META}
    res = {}
    for name in meta:
        m = re.search(r"^" + re.escape(name) + r":[^\n]*\n(.*?)^\.Lfunc_end", text, re.S | re.M)
        body = m.group(1).split("\n")
        cnt = lambda seg, pat: sum(1 for x in instructions(seg) if re.match(pat, x))
        inner = [[x.split()[0] for x in instructions(body[a:b + 1])] for a, b in loops(body, 2) if cnt(body[a:b + 1], r"v_mfma")]
        outer = max(loops(body, 1), key=lambda ab: cnt(body[ab[0]:ab[1] + 1], r"v_mfma"), default=None)
        tl = body[outer[0]:outer[1] + 1] if outer else []
        k_loop = [x.split()[0] for x in instructions(tl)] if not inner and cnt(tl, r"v_mfma") else None
        res[name] = dict(text=re.sub(r"\.LBB\d+_", ".LBB_", m.group(1)), meta=meta[name], inner=inner, k_loop=k_loop,
                         time_loop=len(instructions(tl)), counts={p: cnt(tl, p) for p in COUNTED})
    return res


def short(name):
    """a readable tag of a mangled kernel name: the kernel and its template arguments"""
    m = re.match(r"_ZN4fsnp\d+([a-z0-9_]+?)I(.*)EEvNS_", name)
    if not m:
        return name
    args = re.findall(r"L([ib])(\d+)E", m.group(2))
    return m.group(1) + "<" + ", ".join(("true" if v == "1" else "false") if t == "b" else v for t, v in args) + ">"


EQUAL_META = (".group_segment_fixed_size", ".kernarg_segment_size")
EQUAL_COUNTS = (r"v_mfma", r"buffer_load_dwordx4")


def not_worse(o, n):
    """verdict (iii): see the module's docstring"""
    if o["inner"] or n["inner"]:
        return False
    if any(int(n["meta"][k]) != int(o["meta"][k]) if k in EQUAL_META else int(n["meta"][k]) > int(o["meta"][k]) for k in META):
        return False
    if n["time_loop"] > o["time_loop"]:
        return False
    return all(n["counts"][p] == o["counts"][p] if p in EQUAL_COUNTS else n["counts"][p] <= o["counts"][p] for p in COUNTED)


def compare(old, new, allow_not_worse=False):
    rows, bad = [], 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            rows.append((short(name), "DIFFERENT", "only in " + ("parent" if name in old else "new")))
            bad += 1
            continue
        o, n = old[name], new[name]
        figures = (f"vgpr {n['meta']['.vgpr_count']}, agpr {n['meta']['.agpr_count']}, sgpr {n['meta']['.sgpr_count']}, spills "
                   f"{n['meta']['.vgpr_spill_count']} / {n['meta']['.sgpr_spill_count']}, scratch {n['meta']['.private_segment_fixed_size']}, "
                   f"LDS {n['meta']['.group_segment_fixed_size']}; {len(n['inner'])} k-group loops of "
                   f"{' / '.join(str(len(x)) for x in n['inner']) or '-'}; time loop {o['time_loop']} -> {n['time_loop']}")
        if o["text"] == n["text"] and o["meta"] == n["meta"]:
            rows.append((short(name), "identical", figures))
            continue
        why = [f"{k} {o['meta'][k]} -> {n['meta'][k]}" for k in META if o["meta"][k] != n["meta"][k]]
        if o["inner"] != n["inner"]:
            why.append("k-group loop opcodes differ")
        if o["k_loop"] != n["k_loop"]:
            why.append("depth-1 k-loop opcodes differ")
        if n["time_loop"] > o["time_loop"]:
            why.append(f"time loop {o['time_loop']} -> {n['time_loop']} instructions")
        why += [f"{p} in time loop {o['counts'][p]} -> {n['counts'][p]}" for p in COUNTED if o["counts"][p] != n["counts"][p]]
        changed = sum(1 for a, b in zip(o["text"].split("\n"), n["text"].split("\n")) if a != b) + \
            abs(len(o["text"].split("\n")) - len(n["text"].split("\n")))
        verdict = "(ii)" if not why else "(iii)" if allow_not_worse and not_worse(o, n) else "DIFFERENT"
        rows.append((short(name), verdict, ("; ".join(why) + "; " if why else "") + figures + f"; ~{changed} lines changed"))
        bad += verdict == "DIFFERENT"
    return rows, bad


def main(argv):
    md, allow_not_worse = "--md" in argv, "--not-worse" in argv
    pdir, ndir = [a for a in argv if not a.startswith("--")]
    total_bad = 0
    for fn in sorted(f for f in os.listdir(pdir) if f.endswith(".s")):
        rows, bad = compare(kernels(os.path.join(pdir, fn)), kernels(os.path.join(ndir, fn)), allow_not_worse)
        total_bad += bad
        if md:
            print(f"\n### {fn}\n\n| kernel | verdict | figures (new build) |\n|---|---|---|")
        for r in rows:
            print(f"| `{r[0]}` | {r[1]} | {r[2]} |" if md else f"{fn} {r[0]}: {r[1]}  [{r[2]}]")
    return 1 if total_bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
