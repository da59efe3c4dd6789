#!/usr/bin/env python
"""Instruction census of the innermost loops of one kernel in a gfx950 assembly file.

The two-ended LDS E-step (svae_amd/csrc/lds_estep_twoend.hpp, lds_estep_twoend_s4.hpp) is a latency chain: one
wavefront per SIMD, one instruction every few cycles, so every instruction inside its elimination and smoother
loops costs an issue slot -- scalar instructions, register copies and s_nop included.  This tool prints, per
innermost loop of a kernel, how many instructions of each class one trip issues:

  dpp_fma   v_fmac_f64_dpp / v_fma_f64_dpp (the multiply-accumulates with a row_newbcast operand)
  valu      every other vector ALU instruction (v_mov_b64_dpp, permlane swaps and compares included)
  trans     v_rcp / v_rsq / v_sqrt / v_exp / v_log / v_sin / v_cos
  copy      v_mov_b32 / v_mov_b64 / v_accvgpr_* without a DPP modifier
  s_nop, s_waitcnt, salu (every other scalar instruction, branches included)
  vmem      global_ / buffer_ / flat_ / scratch_ loads and stores
  lds       ds_ instructions

A loop is the span between a label and a later branch back to it; it is innermost when no other such span lies
inside it.  Nothing is executed and nothing is assumed about the trip count: a loop that does four steps per
trip is reported per trip.  Instructions that a forward branch inside the loop jumps over (the elimination loop's
once-per-sequence exchange with the partner chain, its every-fourth-step renormalisation) are counted in `total`
and left out of `hot`, the path every trip takes; the class counts are those of the hot path.

usage: loop_census.py file.s KERNEL [--min N]    KERNEL: a substring of the (mangled) kernel symbol
"""
import re
import sys

CLASSES = ("dpp_fma", "valu", "trans", "copy", "s_nop", "s_waitcnt", "salu", "vmem", "lds")
TRANS = ("v_rcp_", "v_rsq_", "v_sqrt_", "v_exp_", "v_log_", "v_sin_", "v_cos_")
BRANCH = re.compile(r"^s_c?branch\S*\s+(\.L\S+)")


def classify(op):
    """Class of the instruction with mnemonic `op` (None: not an instruction we count, e.g. a directive)."""
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        if op.startswith(("v_fmac_f64_dpp", "v_fma_f64_dpp")):
            return "dpp_fma"
        if op.startswith(TRANS):
            return "trans"
        if "_dpp" not in op and op.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr_")):
            return "copy"
        return "valu"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("ds_"):
        return "lds"
    return None


def kernel_lines(path, kernel):
    """[(line number, text without comment)] of the instructions and labels of the one kernel whose symbol contains
    `kernel`; the symbol.  Raises if no kernel or more than one matches."""
    found, cur, out = [], None, {}
    for ln, line in enumerate(open(path), 1):
        t = line.split(";")[0].strip()
        if not t:
            continue
        if t.endswith(":") and not t.startswith(".L"):
            cur = t[:-1] if kernel in t else None
            if cur is not None:
                found.append(cur)
                out[cur] = []
            continue
        if cur is None:
            continue
        if t.startswith(".") and not t.startswith(".L"):
            if t.startswith((".section", ".rodata", ".amdhsa_kernel")):
                cur = None
            continue
        out[cur].append((ln, t))
    if len(found) != 1:
        raise ValueError("%d kernels match %r: %s" % (len(found), kernel, found[:8]))
    return out[found[0]], found[0]


def innermost_loops(lines):
    """[(index of the label, index of the back edge)] into `lines`, innermost loops only, in program order."""
    label_at = {t[:-1]: i for i, (_, t) in enumerate(lines) if t.endswith(":")}
    spans = []
    for i, (_, t) in enumerate(lines):
        m = BRANCH.match(t)
        if m and m.group(1) in label_at and label_at[m.group(1)] < i:
            spans.append((label_at[m.group(1)], i))
    return [s for s in spans if not any(o != s and s[0] <= o[0] and o[1] <= s[1] for o in spans)]


def census(path, kernel):
    """-> [{"label", "first_line", "last_line", "total", "hot", "counts": {class: n}, "body": [(line, text)]}] per
    innermost loop of the kernel, in program order; `body` and `counts` are the hot path (see above)."""
    lines, _ = kernel_lines(path, kernel)
    out = []
    for a, b in innermost_loops(lines):
        span = lines[a + 1:b + 1]
        label_at = {t[:-1]: i for i, (_, t) in enumerate(span) if t.endswith(":")}
        cold = set()
        for i, (_, t) in enumerate(span):
            m = BRANCH.match(t)
            if m and label_at.get(m.group(1), -1) > i:
                cold.update(range(i + 1, label_at[m.group(1)]))
        is_ins = lambda t: not t.endswith(":") and classify(t.split(None, 1)[0]) is not None
        body = [(ln, t) for i, (ln, t) in enumerate(span) if i not in cold and is_ins(t)]
        counts = dict.fromkeys(CLASSES, 0)
        for _, t in body:
            counts[classify(t.split(None, 1)[0])] += 1
        out.append({"label": lines[a][1][:-1], "first_line": lines[a][0], "last_line": lines[b][0],
                    "total": sum(1 for _, t in span if is_ins(t)), "hot": len(body), "counts": counts, "body": body})
    return out


def main(argv):
    if len(argv) < 3:
        print(__doc__)
        return 2
    least = int(argv[argv.index("--min") + 1]) if "--min" in argv else 0
    _, sym = kernel_lines(argv[1], argv[2])
    print(sym)
    print("%-12s %14s %6s %6s " % ("loop", "lines", "total", "hot") + " ".join("%9s" % c for c in CLASSES))
    for lp in census(argv[1], argv[2]):
        if lp["total"] >= least:
            print("%-12s %6d..%-6d %6d %6d " % (lp["label"], lp["first_line"], lp["last_line"], lp["total"], lp["hot"])
                  + " ".join("%9d" % lp["counts"][c] for c in CLASSES))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
