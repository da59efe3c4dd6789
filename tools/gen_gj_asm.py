#!/usr/bin/env python
"""Generates svae_amd/csrc/gj1r_gen.hpp: the one-register-per-row Gauss-Jordan of the two-ended LDS
E-step kernel (lds_estep_twoend.hpp) with every pivot as ONE hand-scheduled inline-asm block.

Why generated asm: hipcc inserts an s_nop between two inline-asm statements that share a register and
cannot schedule around the DPP / trans hazards inside them, which cost ~85 of ~290 issue slots per
10 x 10 elimination.  Here the row updates themselves provide the wait states:
  * VALU write of a VGPR -> DPP read of it: 2 wait states (two other row updates sit in between);
  * v_rcp_f64 (trans) result -> non-trans VALU use: 1 wait state (one row update in between);
  * the reciprocal chain of the NEXT pivot (v_rcp_f64 + two Newton steps) is interleaved with the row
    updates of the current one, dependent instructions one issue slot apart.
The asm template must be a string literal, hence a generator (python tools/gen_gj_asm.py).
"""
import os

DPP = "row_mask:0xf bank_mask:0xf"
# 1/pn to full fp64 accuracy from the v_rcp_f64 seed t0 (relative error e0 = 1 - pn t0 ~ 2^-23: "2^29 ulp"):
# ONE cubic step  rn = t0 (1 + e0 + e0^2)  -- error e0^3 ~ 2^-69 -- instead of two Newton steps (4 FMAs, 2^-92)
RCP_CHAIN = ["v_rcp_f64 %[t0], %[pn]",
             "v_fma_f64 %[e0], -%[pn], %[t0], 1.0",
             "v_fma_f64 %[e0], %[e0], %[e0], %[e0]",
             "v_fma_f64 %[rn], %[t0], %[e0], %[t0]"]


def pivot_block(N, k):
    """-> (asm lines, has_next).  Operands: %[m0..] rows, %[e] = E[k], %[p], %[ri] in; %[q], %[vf] in/out;
    %[pn], %[rn] out (next pivot, reciprocal); %[ru], %[t0], %[e0] scratch."""
    L = []
    L.append("v_fma_f64 %[ru], -%[p], %[e], %[m{k}]".format(k=k))          # lane k -> exactly 0
    L.append("v_mul_f64 %[ru], %[ru], %[ri]")                               # scaled pivot row
    L.append("v_fma_f64 %[q], %[m{k}], %[ru], %[q]".format(k=k))
    L.append("v_fma_f64 %[vf], -%[ri], %[e], %[vf]")
    upd = lambda i: "v_fmac_f64_dpp %[m{i}], %[m{i}], -%[ru] row_newbcast:{k} {d}".format(i=i, k=k, d=DPP)
    if k + 1 < N:
        others = list(range(k + 2, N)) + list(range(0, k))
        L.append(upd(k + 1))
        pre = others[:2]
        others = others[2:]
        for i in pre:
            L.append(upd(i))
        if len(pre) < 2:
            L.append("s_nop %d" % (1 - len(pre)))
        L.append("v_mov_b64_dpp %[pn], %[m{i}] row_newbcast:{i} {d}".format(i=k + 1, d=DPP))
        chain = RCP_CHAIN
        for ci, ins in enumerate(chain):
            L.append(ins)
            if ci < len(chain) - 1:
                if others:
                    L.append(upd(others.pop(0)))
                elif ci == 0:
                    L.append("s_nop 0")            # trans result -> VALU use
        for i in others:
            L.append(upd(i))
        L.append("v_add_f64 %[m{k}], %[ru], -%[e]".format(k=k))            # pivot row as kept: lane k = -1
        return L, True
    for i in range(0, N - 1):
        L.append(upd(i))
    L.append("v_add_f64 %[m{k}], %[ru], -%[e]".format(k=k))
    return L, False


def emit(N, rows=False):
    """rows: the variant that also returns every scaled pivot row (RU[k]; lanes j > k: L[j][k], the unit LDL' factor
    the backward sampler reads -- lds_filter_1r.hpp)."""
    out = []
    out.append("template <>")
    if rows:
        out.append("__device__ __forceinline__ void gauss_jordan_1r_asm_rows<%d>(double (&M)[%d], const double (&E)[%d], "
                   "double& qacc, double& vfull, double (&RU)[%d]) {" % (N, N, N, N))
    else:
        out.append("__device__ __forceinline__ void gauss_jordan_1r_asm<%d>(double (&M)[%d], const double (&E)[%d], "
                   "double& qacc, double& vfull) {" % (N, N, N))
    out.append("  double p = bcast_fenced<0>(M[0]);")
    out.append("  double rinv = rcp_nr(p);")
    out.append("  double %st0, e0, pn, rn;" % ("" if rows else "ru, "))
    out.append("  (void)t0; (void)e0; (void)pn; (void)rn;")
    for k in range(N):
        lines, has_next = pivot_block(N, k)
        body = "\\n\\t\"\n      \"".join(lines)
        rowops = ", ".join('[m%d] "+v"(M[%d])' % (i, i) for i in range(N))
        outs = rowops + ', [q] "+v"(qacc), [vf] "+v"(vfull), [ru] "=&v"(%s)' % ("RU[%d]" % k if rows else "ru")
        if has_next:
            outs += ', [t0] "=&v"(t0), [e0] "=&v"(e0), [pn] "=&v"(pn), [rn] "=&v"(rn)'
        ins = '[e] "v"(E[%d]), [p] "v"(p), [ri] "v"(rinv)' % k
        out.append("  asm volatile(\n      \"%s\"\n      : %s\n      : %s);" % (body, outs, ins))
        if has_next:
            out.append("  p = pn; rinv = rn;")
    out.append("}")
    return "\n".join(out)


def pivot_block2(N, k):
    """Two registers per row (row-per-chain layout, lds_estep_twoend_rpc.hpp): a_i = [P row | .. | h] (lanes < N, lane
    15), b_i = right-hand-side columns (lanes < N).  Row update = two DPP FMAs, both broadcasting the multiplier
    f_i = lane k of a_i: the b update first (the a update rewrites a_i; its lane k keeps f_i because ru lane k = 0).
    Operands as pivot_block plus %[b0..]; the scaled pivot row of the b set is formed in place (b_k *= 1/p_k)."""
    L = []
    L.append("v_fma_f64 %[ru], -%[p], %[e], %[a{k}]".format(k=k))          # lane k -> exactly 0
    L.append("v_mul_f64 %[b{k}], %[b{k}], %[ri]".format(k=k))               # scaled pivot row, b set (in place)
    L.append("v_mul_f64 %[ru], %[ru], %[ri]")                               # scaled pivot row, a set
    L.append("v_fma_f64 %[vf], -%[ri], %[e], %[vf]")
    L.append("v_fma_f64 %[q], %[a{k}], %[ru], %[q]".format(k=k))
    updb = lambda i: "v_fmac_f64_dpp %[b{i}], %[a{i}], -%[b{k}] row_newbcast:{k} {d}".format(i=i, k=k, d=DPP)
    upda = lambda i: "v_fmac_f64_dpp %[a{i}], %[a{i}], -%[ru] row_newbcast:{k} {d}".format(i=i, k=k, d=DPP)
    others = list(range(k + 2, N)) + list(range(0, k))
    work = []
    for i in others:
        work += [updb(i), upda(i)]
    if k + 1 < N:
        L += [updb(k + 1), upda(k + 1)]
        pre = work[:2]
        work = work[2:]
        L += pre
        if len(pre) < 2:
            L.append("s_nop %d" % (1 - len(pre)))
        L.append("v_mov_b64_dpp %[pn], %[a{i}] row_newbcast:{i} {d}".format(i=k + 1, d=DPP))
        for ci, ins in enumerate(RCP_CHAIN):
            L.append(ins)
            if ci < len(RCP_CHAIN) - 1:
                if work:
                    L.append(work.pop(0))
                elif ci == 0:
                    L.append("s_nop 0")            # trans result -> VALU use
        L += work
        L.append("v_add_f64 %[a{k}], %[ru], -%[e]".format(k=k))            # pivot row as kept: lane k = -1
        return L, True
    L += work
    L.append("v_add_f64 %[a{k}], %[ru], -%[e]".format(k=k))
    return L, False


def emit2(N):
    out = []
    out.append("template <>")
    out.append("__device__ __forceinline__ void gauss_jordan_2r_asm<%d>(double (&A)[%d], double (&B)[%d], const double (&E)[%d], "
               "double& qacc, double& vfull) {" % (N, N, N, N))
    out.append("  double p = bcast_fenced<0>(A[0]);")
    out.append("  double rinv = rcp_nr(p);")
    out.append("  double ru, t0, e0, pn, rn;")
    out.append("  (void)t0; (void)e0; (void)pn; (void)rn;")
    for k in range(N):
        lines, has_next = pivot_block2(N, k)
        body = "\\n\\t\"\n      \"".join(lines)
        rowops = ", ".join('[a%d] "+v"(A[%d])' % (i, i) for i in range(N)) + ", " + \
            ", ".join('[b%d] "+v"(B[%d])' % (i, i) for i in range(N))
        outs = rowops + ', [q] "+v"(qacc), [vf] "+v"(vfull), [ru] "=&v"(ru)'
        if has_next:
            outs += ', [t0] "=&v"(t0), [e0] "=&v"(e0), [pn] "=&v"(pn), [rn] "=&v"(rn)'
        ins = '[e] "v"(E[%d]), [p] "v"(p), [ri] "v"(rinv)' % k
        out.append("  asm volatile(\n      \"%s\"\n      : %s\n      : %s);" % (body, outs, ins))
        if has_next:
            out.append("  p = pn; rinv = rn;")
    out.append("}")
    return "\n".join(out)


# ---- the elimination step of the two-ended kernel as three blocks (lds_estep_twoend.hpp: elim_step) ----------------
# hipcc pads between separate inline-asm statements that share a register (an s_nop after every second multiply-add
# of a product stage, one between two pivot blocks) and cannot start the first pivot's reciprocal before the
# statements in front of it are through.  One statement per stage leaves it nothing to pad; the wait states a
# DPP / trans hazard does need are counted here (tools/audit_dpp_hazards.py checks the result).

def condition_block(N):
    """Adds the node's potential vector to lane 15 of every row (M[i] += bcast_i(ho) * EH, as mac_bc<i>) and starts the
    Gauss-Jordan's FIRST pivot on the way: p = M[0][0] is final after the first of these multiply-adds, so its
    broadcast and the reciprocal chain (the arithmetic of rcp_nr, dpp.hpp) ride between the others instead of standing
    alone, serial, in front of the first pivot block."""
    mac = lambda i: "v_fmac_f64_dpp %[m{i}], %[ho], %[eh] row_newbcast:{i} {d}".format(i=i, d=DPP)
    fill = [mac(i) for i in range(1, N)]
    L = [mac(0)]

    def wait(states):            # `states` wait states from other work, s_nop for what is missing
        got = 0
        while got < states and fill:
            L.append(fill.pop(0))
            got += 1
        if got < states:
            L.append("s_nop %d" % (states - got - 1))

    wait(2)                                                                 # VALU write of m0 -> DPP read
    L.append("v_mov_b64_dpp %[p], %[m0] row_newbcast:0 {d}".format(d=DPP))
    L.append("v_rcp_f64 %[t0], %[p]")
    wait(1)                                                                 # trans result -> VALU use
    for _ in range(2):                                                      # (its latency is about two FMAs')
        if fill:
            L.append(fill.pop(0))
    L.append("v_fma_f64 %[e0], -%[p], %[t0], 1.0")
    if fill:
        L.append(fill.pop(0))
    L.append("v_fma_f64 %[e0], %[e0], %[e0], %[e0]")
    if fill:
        L.append(fill.pop(0))
    L.append("v_fma_f64 %[ri], %[t0], %[e0], %[t0]")
    return L + fill


def emit_condition(N):
    out = ["template <>",
           "__device__ __forceinline__ void te_condition_asm<%d>(double (&M)[%d], double ho, double EH, double& p, "
           "double& rinv) {" % (N, N),
           "  double t0, e0;"]
    body = "\\n\\t\"\n      \"".join(condition_block(N))
    outs = ", ".join('[m%d] "+v"(M[%d])' % (i, i) for i in range(N))
    outs += ', [p] "=&v"(p), [ri] "=&v"(rinv), [t0] "=&v"(t0), [e0] "=&v"(e0)'
    out.append("  asm volatile(\n      \"%s\"\n      : %s\n      : [ho] \"v\"(ho), [eh] \"v\"(EH));" % (body, outs))
    out.append("}")
    return "\n".join(out)


def emit_from_pivot(N):
    """gauss_jordan_1r_asm with the first pivot and its reciprocal handed in, every pivot in ONE statement.  The
    arithmetic per element is pivot_block()'s; with the blocks in one statement their instructions can be placed for
    latency across the block boundary:
      * the head of block k + 1 -- its scaled pivot row ru = (M[k+1] - p e) * (1/p), two dependent instructions every
        row update of that block waits for -- is issued inside block k (row k + 1 is final after the block's first
        update, p after the broadcast, 1/p after the chain); the pivot row alternates between two registers, like
        the (pivot, reciprocal) pair;
      * v_rcp_f64 has about twice the latency of an FMA: three instructions stand between it and its first use, one
        between the dependent FMAs behind it."""
    sets = [("%[p]", "%[ri]"), ("%[pa]", "%[ra]"), ("%[pb]", "%[rb]")]
    rus = ["%[ru]", "%[rv]"]
    lines = []
    for k in range(N):
        p, ri = sets[0] if k == 0 else sets[1 + (k - 1) % 2]
        pn, rn = sets[1 + k % 2]
        ru, run = rus[k % 2], rus[(k + 1) % 2]
        e, en, mk = "%%[u%d]" % k, "%%[u%d]" % (k + 1), "%%[m%d]" % k
        upd = lambda i: "v_fmac_f64_dpp %[m{i}], %[m{i}], -{ru} row_newbcast:{k} {d}".format(i=i, ru=ru, k=k, d=DPP)
        L = []
        if k == 0:
            L.append("v_fma_f64 %s, -%s, %s, %s" % (ru, p, e, mk))         # lane k -> exactly 0
            L.append("v_mul_f64 %s, %s, %s" % (ru, ru, ri))                 # scaled pivot row
        L.append("v_fma_f64 %[q], {m}, {ru}, %[q]".format(m=mk, ru=ru))
        L.append("v_fma_f64 %[vf], -{ri}, {e}, %[vf]".format(ri=ri, e=e))
        if k + 1 < N:
            others = [upd(i) for i in list(range(k + 2, N)) + list(range(0, k))]
            take = lambda n: [others.pop(0) for _ in range(min(n, len(others)))]
            L.append(upd(k + 1))
            pre = take(2)
            L += pre
            if len(pre) < 2:
                L.append("s_nop %d" % (1 - len(pre)))                       # VALU write -> DPP read: 2 wait states
            L.append("v_mov_b64_dpp {pn}, %[m{i}] row_newbcast:{i} {d}".format(pn=pn, i=k + 1, d=DPP))
            L.append("v_rcp_f64 %[t0], " + pn)
            L += take(2)
            L.append("v_fma_f64 %s, -%s, %s, %%[m%d]" % (run, pn, en, k + 1))   # next block's head (also the trans wait state)
            L.append("v_fma_f64 %[e0], -" + pn + ", %[t0], 1.0")
            L += take(1)
            L.append("v_fma_f64 %[e0], %[e0], %[e0], %[e0]")
            L += take(1)
            L.append("v_fma_f64 " + rn + ", %[t0], %[e0], %[t0]")
            L += take(1)
            L.append("v_mul_f64 %s, %s, %s" % (run, run, rn))
            L += others
        else:
            L += [upd(i) for i in range(0, N - 1)]
        L.append("v_add_f64 %s, %s, -%s" % (mk, ru, e))                     # pivot row as kept: lane k = -1
        lines += L
    out = ["template <>",
           "__device__ __forceinline__ void gauss_jordan_1r_asm_from<%d>(double (&M)[%d], const double (&E)[%d], "
           "double& qacc, double& vfull, double p, double rinv) {" % (N, N, N),
           "  double ru, rv, t0, e0, pa, ra, pb, rb;",
           "  (void)rv; (void)t0; (void)e0; (void)pa; (void)ra; (void)pb; (void)rb;"]
    body = "\\n\\t\"\n      \"".join(lines)
    outs = ", ".join('[m%d] "+v"(M[%d])' % (i, i) for i in range(N))
    outs += ', [q] "+v"(qacc), [vf] "+v"(vfull), [ru] "=&v"(ru)'
    if N > 1:
        outs += ', [rv] "=&v"(rv), [t0] "=&v"(t0), [e0] "=&v"(e0), [pa] "=&v"(pa), [ra] "=&v"(ra)'
    if N > 2:
        outs += ', [pb] "=&v"(pb), [rb] "=&v"(rb)'
    ins = ", ".join('[u%d] "v"(E[%d])' % (k, k) for k in range(N)) + ', [p] "v"(p), [ri] "v"(rinv)'
    out.append("  asm volatile(\n      \"%s\"\n      : %s\n      : %s);" % (body, outs, ins))
    out.append("}")
    return "\n".join(out)


def emit_schur(N):
    """The Schur stage  AnD[j] += bcast_{N+j}(M[k]) * Bt[k]  (k outer, j inner: the order of the mac_bc statements it
    replaces) as one statement.  M[k] is the DPP operand: the Gauss-Jordan's last block writes M[0] .. M[N-2] in this
    order and M[N-1] last of all, so only N <= 2 needs wait states in front (an instruction between the two
    statements only adds to them)."""
    J = (N + 1) // 2
    L = []
    if N <= 2:
        L.append("s_nop %d" % (2 - N))
    for k in range(N):
        for j in range(J):
            L.append("v_fmac_f64_dpp %[a{j}], %[m{k}], %[b{k}] row_newbcast:{l} {d}".format(j=j, k=k, l=N + j, d=DPP))
    out = ["template <>",
           "__device__ __forceinline__ void te_schur_asm<%d>(double (&AnD)[%d], const double (&M)[%d], "
           "const double (&Bt)[%d]) {" % (N, J, N, N)]
    body = "\\n\\t\"\n      \"".join(L)
    outs = ", ".join('[a%d] "+v"(AnD[%d])' % (j, j) for j in range(J))
    ins = ", ".join('[m%d] "v"(M[%d])' % (k, k) for k in range(N)) + ", " + \
        ", ".join('[b%d] "v"(Bt[%d])' % (k, k) for k in range(N))
    out.append("  asm volatile(\n      \"%s\"\n      : %s\n      : %s);" % (body, outs, ins))
    out.append("}")
    return "\n".join(out)


# ---- the product stages of the one-chain-per-wavefront smoother step (lds_estep_twoend_s4.hpp: pstep) ----------------
# Four-row slot layout: row i of a tile lives in DPP row i & 3, slot i >> 2; J = (N + 3) / 4 slots hold rows 0 .. N-1,
# J1 = (N + 4) / 4 rows 0 .. N.  As separate mac_bc statements hipcc padded one of the four unrolled steps of the
# loop with an s_nop behind every `k` group (22 per trip at N = 10), although the DPP operand of a stage is never
# written inside it.  Order: k outer, j inner -- the order of the statements they replace.

def smoother_stage(N, kind):
    """-> (lines, number of accumulators, number of b operands).  acc[j] += bcast_k(d[j]) * (+/-) b[k]:
      "w":    W~ = S~ G~'        acc = W (J1),  d = S~ (J1),   b = H[0..N]  (the transposed G~; - for k < N, + for row N)
      "prep": G~ = P^-1 NJ12c    acc = Gc (J),  d = Pi (J),    b = NJ12c[0..N-1]  (-)
      "s":    S~ = PiZ + G~ W~   acc = PiZ (J1), d = Gc (J1),  b = WR[0..N]  (- for k < N, + for row N)
    Wait states (VALU write of a VGPR -> DPP read of it: 2).  "prep" and "s" read registers written a whole step
    earlier (the record; the preparation of this step, issued during the previous one).  "w" reads S~, which the "s"
    statement of the previous step wrote LAST: slot j in the last J1 - j instructions of that statement, read here by
    instruction j of the first group -- J1 - 1 instructions lie between the write of a slot and its read even when the
    two statements are adjacent, so only J1 < 3 needs s_nop in front (anything between the statements adds to it)."""
    J, J1 = (N + 3) // 4, (N + 4) // 4
    nacc, nb = (J, N) if kind == "prep" else (J1, N + 1)
    L = []
    if kind == "w" and J1 < 3:
        L.append("s_nop %d" % (2 - J1))
    for k in range(nb):
        sign = "-" if (kind == "prep" or k < N) else ""
        for j in range(nacc):
            L.append("v_fmac_f64_dpp %[a{j}], %[d{j}], {s}%[b{k}] row_newbcast:{k} {d}".format(j=j, k=k, s=sign, d=DPP))
    return L, nacc, nb


def emit_smoother_stage(N, kind):
    J1 = (N + 4) // 4
    L, nacc, nb = smoother_stage(N, kind)
    nbdecl = {"w": N + 1, "prep": N, "s": N + 2}[kind]       # ("s": the gathered tile is read in pairs, N + 2 registers)
    out = ["template <>",
           "__device__ __forceinline__ void te_smooth_%s_asm<%d>(double (&A)[%d], const double (&D)[%d], "
           "const double (&Bk)[%d]) {" % (kind, N, J1, J1, nbdecl)]
    body = "\\n\\t\"\n      \"".join(L)
    outs = ", ".join('[a%d] "+v"(A[%d])' % (j, j) for j in range(nacc))
    ins = ", ".join('[d%d] "v"(D[%d])' % (j, j) for j in range(nacc)) + ", " + \
        ", ".join('[b%d] "v"(Bk[%d])' % (k, k) for k in range(nb))
    out.append("  asm volatile(\n      \"%s\"\n      : %s\n      : %s);" % (body, outs, ins))
    out.append("}")
    return "\n".join(out)


HEADER = '''// gj1r_gen.hpp -- GENERATED by tools/gen_gj_asm.py; do not edit.
// In-place Gauss-Jordan on one register per row (see gauss_jordan_1r in lds_estep_twoend.hpp for the
// algorithm and the meaning of the operands), one hand-scheduled inline-asm block per pivot.
#pragma once
#include "dpp.hpp"

namespace svae {

template <int N>
__device__ __forceinline__ void gauss_jordan_1r_asm(double (&M)[N], const double (&E)[N], double& qacc,
                                                    double& vfull);
// the same, also returning the scaled pivot rows (RU[k], lanes j > k: L[j][k])
template <int N>
__device__ __forceinline__ void gauss_jordan_1r_asm_rows(double (&M)[N], const double (&E)[N], double& qacc,
                                                         double& vfull, double (&RU)[N]);
// two registers per row (row-per-chain layout, lds_estep_twoend_rpc.hpp): A = [P | h], B = right-hand-side columns
template <int N>
__device__ __forceinline__ void gauss_jordan_2r_asm(double (&A)[N], double (&B)[N], const double (&E)[N], double& qacc,
                                                    double& vfull);
// the elimination step of the two-ended kernel, one statement per stage: the node potential's conditioning with the
// first pivot's reciprocal started inside it, the Gauss-Jordan from that pivot on, the Schur stage
template <int N>
__device__ __forceinline__ void te_condition_asm(double (&M)[N], double ho, double EH, double& p, double& rinv);
template <int N>
__device__ __forceinline__ void gauss_jordan_1r_asm_from(double (&M)[N], const double (&E)[N], double& qacc,
                                                         double& vfull, double p, double rinv);
template <int N>
__device__ __forceinline__ void te_schur_asm(double (&AnD)[(N + 1) / 2], const double (&M)[N], const double (&Bt)[N]);
// the product stages of the one-chain-per-wavefront smoother step (lds_estep_twoend_s4.hpp), four-row slot layout,
// one statement each:  A[j] += bcast_k(D[j]) * (+/-) Bk[k],  k outer, j inner
//   w:    W~ = S~ G~'        A = W,       D = S~,    Bk = H (G~ transposed, replicated)
//   prep: G~ = P^-1 NJ12c    A = G~ rows, D = P^-1,  Bk = NJ12c        (rows 0 .. N-1 only)
//   s:    S~ = PiZ + G~ W~   A = PiZ,     D = G~,    Bk = the gathered W~
template <int N>
__device__ __forceinline__ void te_smooth_w_asm(double (&A)[(N + 4) / 4], const double (&D)[(N + 4) / 4],
                                                const double (&Bk)[N + 1]);
template <int N>
__device__ __forceinline__ void te_smooth_prep_asm(double (&A)[(N + 4) / 4], const double (&D)[(N + 4) / 4],
                                                   const double (&Bk)[N]);
template <int N>
__device__ __forceinline__ void te_smooth_s_asm(double (&A)[(N + 4) / 4], const double (&D)[(N + 4) / 4],
                                                const double (&Bk)[N + 2]);

'''

def generate():
    """The whole header as a string (tests/test_build_audit.py diffs it against the committed file)."""
    parts = [HEADER]
    for N in range(1, 11):
        parts.append(emit(N) + "\n\n")
        parts.append(emit(N, rows=True) + "\n\n")
        parts.append(emit2(N) + "\n\n")
        parts.append(emit_condition(N) + "\n\n")
        parts.append(emit_from_pivot(N) + "\n\n")
        parts.append(emit_schur(N) + "\n\n")
        for kind in ("w", "prep", "s"):
            parts.append(emit_smoother_stage(N, kind) + "\n\n")
    parts.append("}  // namespace svae\n")
    return "".join(parts)


if __name__ == "__main__":
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "svae_amd", "csrc", "gj1r_gen.hpp")
    with open(path, "w") as f:
        f.write(generate())
    print("wrote", path)
