"""Instruction mix of the loop blocks of the factorisation's product kernels, from the gfx950 assembly of mf_numeric.hip:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -munsafe-fp-atomics -ffp-contract=fast -Iinclude -Iipc_amd/csrc -x hip --cuda-device-only -S \
        ipc_amd/csrc/mf_numeric.hip -o mf_numeric.s
    python tools/loop_instruction_counts.py mf_numeric.s [kernel name fragment ...]

For every innermost loop that holds MFMAs (its blocks from the header to the last branch back to it): MFMAs, global loads, other VALU, SALU, waits and
the instructions the loop of a full chunk should not need (v_cndmask, v_min, 64-bit multiplies, accumulator copies).  A record for profiles/, not a test."""
import re
import sys

KERNELS = ("k_big_schur64_ea", "k_big_schur64", "k_big_schurE", "k_big_bulk", "k_xinv_gemm", "k_big_step")


def kernels(lines):
    name, body = None, []
    for ln in lines:
        m = re.match(r"^(_Z\w+):", ln)
        if m:
            name, body = m.group(1), []
        elif name and ln.startswith(".Lfunc_end"):
            yield name, body
            name = None
        elif name:
            body.append(ln)


def blocks(body):
    label, cur = "entry", []
    for ln in body:
        m = re.match(r"^(\.LBB\w+):", ln)
        if m:
            yield label, cur
            label, cur = m.group(1), []
        else:
            s = ln.split(";")[0].strip()
            if s and not s.startswith("."):
                cur.append(s)
    yield label, cur


def classify(ins):
    op = ins.split()[0]
    if op.startswith("v_mfma"):
        return "mfma"
    if op.startswith("global_load") or op.startswith("buffer_load") or op.startswith("flat_load"):
        return "load"
    if op.startswith("global_store") or op.startswith("ds_"):
        return "other_mem"
    if op.startswith("s_waitcnt") or op.startswith("s_nop"):
        return "wait"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "other"


def loops(body):
    """innermost loops as (header label, instructions): the blocks from a label up to the LAST branch back to it, when no other loop header lies between
    (a conditional block in the middle of a loop body is counted with it)"""
    bl = list(blocks(body))
    labels = [b[0] for b in bl]
    for i, (label, _) in enumerate(bl):
        last = -1
        for j in range(i, len(bl)):
            if any(x.startswith(("s_cbranch", "s_branch")) and x.split()[-1] == label for x in bl[j][1]):
                last = j
        if last < 0:
            continue
        inner = False
        for k in range(i + 1, last + 1):  # another back edge inside: not innermost
            if any(x.startswith(("s_cbranch", "s_branch")) and x.split()[-1] in labels[i + 1:k + 1] for x in bl[k][1]):
                inner = True
        if not inner:
            yield label, [x for b in bl[i:last + 1] for x in b[1]], last - i + 1


def main():
    lines = open(sys.argv[1]).read().splitlines()
    want = sys.argv[2:] or KERNELS
    for name, body in kernels(lines):
        if not any(w in name for w in want):
            continue
        for label, ins, nb in loops(body):
            c = {}
            for i in ins:
                c[classify(i)] = c.get(classify(i), 0) + 1
            if not c.get("mfma"):
                continue
            cnd = sum(i.startswith("v_cndmask") for i in ins)
            vmin = sum(i.startswith("v_min") for i in ins)
            mul64 = sum(i.startswith(("v_mad_u64", "v_mad_i64", "v_mul_lo", "v_mul_hi")) for i in ins)
            acc = sum(i.startswith("v_accvgpr") for i in ins)
            short = re.sub(r"^_ZN6ipcgpu12_GLOBAL__N_1\d+", "", name)[:24]
            print(f"{short} {label} ({nb} block{'s' if nb > 1 else ''}): {len(ins)} instructions | mfma {c.get('mfma', 0)} loads {c.get('load', 0)} other VALU {c.get('valu', 0)} "
                  f"(v_cndmask {cnd}, v_min {vmin}, 64-bit multiplies {mul64}, accvgpr copies {acc}) SALU {c.get('salu', 0)} waits/nops {c.get('wait', 0)} "
                  f"other {c.get('other_mem', 0) + c.get('other', 0)}")


if __name__ == "__main__":
    main()
