#!/usr/bin/env python3
"""Build-time check of the inline-assembly granule loads (grid_sync.hpp / solver_pipe.hpp load_pair).

`load_pair` issues `global_load_dwordx4 vDST, vADDR, off sc1` from inline asm; the compiler's own wait counting does
not see it, so the code relies on every such load being followed by an explicit `s_waitcnt vmcnt(0)` BEFORE any
instruction reads or overwrites vDST.  That holds by construction of the source and by register allocation; this
script verifies it in the ISA actually built: it extracts the gfx950 code object from the object file / library,
disassembles it and walks every such load forward, along every path of the control flow, to the wait that covers it -- `s_waitcnt
vmcnt(0)`, or the counted wait of the collector's poll ring (see check()) -- failing if any instruction in between names one of the
four destination registers; a path that reaches the end of the program first is reported.

    python tools/check_async_loads.py [object files; default: rdis_amd/lib/obj/rdis_hip.o and refround_kernels.o]
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def disassemble(obj):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        return subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], check=True, capture_output=True, text=True).stdout


def regs_of(tok):
    """the vector registers an operand token names: v12 -> {12}, v[4:7] -> {4, 5, 6, 7}"""
    m = re.fullmatch(r"v(\d+)", tok)
    if m:
        return {int(m.group(1))}
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    return set()


def check(text):
    """Every path from a load is followed through the control flow (both ways at a conditional branch, to the target of an
    unconditional one) up to a wait that proves the load has landed: `s_waitcnt vmcnt(0)`, or a counted `s_waitcnt vmcnt(N)`
    (the collector's poll ring, solver_pipe.hpp: sweep_ring) once at least N vector-memory loads were issued after this one on
    the path -- loads return in order among loads, so N or fewer operations outstanding then leaves this one none of them.
    A path that reaches the end of the program (or an indirect jump) first is counted as open-ended."""
    loads, bad, open_ended = 0, [], 0
    lines = text.splitlines()
    insn = re.compile(r"^\s+([a-z_0-9]+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):")
    parsed, at, funcs = [None] * len(lines), {}, ["?"] * len(lines)
    func = "?"
    for i, ln in enumerate(lines):
        m = re.match(r"^[0-9a-f]+ <(.+)>:", ln)
        if m:
            func = m.group(1)
        funcs[i] = func
        m = insn.match(ln)
        if m:
            parsed[i] = (m.group(1), m.group(2), int(m.group(3), 16))
            at[int(m.group(3), 16)] = i

    def is_poll(op, rest):
        return op == "global_load_dwordx4" and " sc1" in " " + rest

    def target(rest, addr):
        simm = int(rest.split()[0]) & 0xFFFF
        return at.get(addr + 4 + 4 * (simm - 0x10000 if simm & 0x8000 else simm))

    def nxt(i):
        i += 1
        while i < len(lines) and parsed[i] is None:
            i += 1
        return i if i < len(lines) else None

    # The compiler gives a loop with several ways out ONE exit: a way out sets a flag in scalar registers and jumps to a block
    # that tests it.  Followed blindly, such a block leads from every way out back into the loop, on paths no wave takes.
    # So the walk carries what it knows of the scalar registers -- constants moved in, and the scc / vcc formed from them --
    # and takes only the side of a branch that those decide.  Anything else written to a scalar register forgets it.
    M32 = 0xFFFFFFFF

    def sregs(tok):
        tok = tok.strip()
        m = re.fullmatch(r"s(\d+)", tok)
        if m:
            return [int(m.group(1))]
        m = re.fullmatch(r"s\[(\d+):(\d+)\]", tok)
        if m:
            return list(range(int(m.group(1)), int(m.group(2)) + 1))
        return []

    def imm(tok):
        tok = tok.strip()
        try:
            return int(tok, 0) & M32
        except ValueError:
            return None

    def val32(st, tok):
        r = sregs(tok)
        if len(r) == 1:
            return st.get(r[0])
        return imm(tok)

    VCC_PARTS = ("vcc", "vcc_lo", "vcc_hi")
    NO_SCALAR_WRITE = ("s_cbranch", "s_branch", "s_waitcnt", "s_sleep", "s_nop", "s_barrier", "s_setprio", "s_endpgm", "s_dcache_inv", "s_icache_inv")
    # scalar ALU and scalar loads whose one destination is the first operand (plus, for most, scc)
    SALU_DST_FIRST = re.compile(r"s_(add|addc|sub|subb|and|or|xor|andn2|orn2|nand|nor|xnor|lshl|lshr|ashr|min|max|mul|mul_hi|bfe|bfm|not|brev|"
                                r"bcnt[01]|ff[01]|flbit|sext|abs|absdiff|lshl[1-4]_add|cselect|mov|cmov|movk|addk|mulk|[a-z0-9]+_saveexec|"
                                r"load|buffer_load|memtime|memrealtime|getpc)_[a-z0-9_]+")
    KEEPS_SCC = ("s_mov_b32", "s_mov_b64", "s_cselect_b32", "s_cselect_b64", "s_memtime", "s_memrealtime", "s_getpc_b64")

    def step(st, op, rest):
        """the scalar state after the instruction (a dict: register number -> 32-bit constant, 'scc' -> 0 / 1, 'vcc' -> 'z' / 'nz').
        Only what is listed here is modelled; any other instruction that is scalar, or that names a scalar register, vcc or exec
        among its first two operands (where a vector instruction's scalar results stand), forgets everything: a path is never
        dropped on knowledge that an instruction this model does not understand could have made stale."""
        ops = [t.strip() for t in rest.split(",")] if rest else []
        if op.startswith(NO_SCALAR_WRITE):
            return st
        st = dict(st)
        if op.startswith("s_cmp_") and len(ops) == 2:
            x, y = val32(st, ops[0]), val32(st, ops[1])
            st.pop("scc", None)
            if x is not None and y is not None:
                sg = lambda v: v - (1 << 32) if v & 0x80000000 else v
                if op.endswith("_i32"):
                    x, y = sg(x), sg(y)
                rel = op[len("s_cmp_"):-4]
                res = {"eq": x == y, "lg": x != y, "gt": x > y, "ge": x >= y, "lt": x < y, "le": x <= y}.get(rel)
                if res is not None:
                    st["scc"] = int(res)
            return st
        if op.startswith(("s_bitcmp", "s_cmpk_")):
            st.pop("scc", None)
            return st
        if op.startswith("s_"):
            if not SALU_DST_FIRST.fullmatch(op) or not ops:
                return {}
            dst = ops[0]
            scc_in = st.get("scc")
            if op not in KEEPS_SCC and not op.startswith(("s_load", "s_buffer_load")):
                st.pop("scc", None)
            if dst in VCC_PARTS:
                st.pop("vcc", None)
                if dst == "vcc" and op in ("s_andn2_b64", "s_and_b64") and len(ops) == 3 and ops[1] == "exec":
                    r = sregs(ops[2])
                    if len(r) == 2 and st.get(r[0]) in (0, M32) and st.get(r[0]) == st.get(r[1]):
                        ones = st[r[0]] == M32
                        st["vcc"] = ("z" if ones else "nz") if op == "s_andn2_b64" else ("nz" if ones else "z")
                return st
            regs = sregs(dst)
            if not regs:
                return {}      # (exec, m0, ttmp...: not modelled)
            for r in regs:
                st.pop(r, None)
            if op == "s_mov_b32" and len(regs) == 1 and len(ops) == 2:
                v = val32(st, ops[1])
                if v is not None:
                    st[regs[0]] = v
            elif op == "s_mov_b64" and len(regs) == 2 and len(ops) == 2:
                v = imm(ops[1])
                if v in (0, M32):
                    st[regs[0]] = st[regs[1]] = v
            elif op == "s_cselect_b64" and len(regs) == 2 and len(ops) == 3 and scc_in is not None:
                v = imm(ops[1] if scc_in else ops[2])
                if v in (0, M32):
                    st[regs[0]] = st[regs[1]] = v
            return st
        # vector, LDS and memory instructions: a scalar result stands among the first two operands (v_cmp_e32: vcc, unnamed)
        if op.startswith("v_cmp") or op.startswith(("v_readfirstlane", "v_readlane")):
            return {}
        for t in ops[:2]:
            if t in VCC_PARTS or t.startswith("exec") or sregs(t):
                return {}
        return st

    def taken(st, op):
        """True / False where the state decides a conditional branch, None where it does not"""
        if op == "s_cbranch_scc0" and "scc" in st:
            return st["scc"] == 0
        if op == "s_cbranch_scc1" and "scc" in st:
            return st["scc"] == 1
        if op == "s_cbranch_vccz" and "vcc" in st:
            return st["vcc"] == "z"
        if op == "s_cbranch_vccnz" and "vcc" in st:
            return st["vcc"] == "nz"
        return None

    for i, pi in enumerate(parsed):
        if pi is None or not is_poll(pi[0], pi[1]):
            continue
        dst = regs_of(pi[1].split(",")[0].strip())
        if len(dst) != 4:
            continue
        loads += 1
        seen, todo, verdict = set(), [(nxt(i), 0, {})], None
        while todo and verdict is None:
            j, later, st = todo.pop()
            if j is None:
                verdict = "open"
                break
            key = (j, later, frozenset(st.items()))
            if key in seen:
                continue
            seen.add(key)
            if len(seen) > 2000000:
                verdict = "open"     # (gave up: reported, not passed)
                break
            op, rest, addr = parsed[j]
            if op == "s_waitcnt":
                m = re.search(r"vmcnt\((\d+)\)", rest)
                if m and later >= int(m.group(1)):
                    continue      # landed on this path
            if op in ("s_endpgm", "s_setpc_b64", "s_swappc_b64"):
                verdict = "open"
                break
            used = set()
            for t in re.findall(r"v\[\d+:\d+\]|v\d+", rest):
                used |= regs_of(t)
            if used & dst:
                bad.append((funcs[i], lines[i].strip(), lines[j].strip()))
                verdict = "bad"
                break
            if op.startswith(("global_load", "buffer_load", "flat_load", "scratch_load")):
                later = min(later + 1, 64)
            if op == "s_branch":
                todo.append((target(rest, addr), later, st))
                continue
            if op.startswith("s_cbranch"):
                t = taken(st, op)
                if t is not False:
                    todo.append((target(rest, addr), later, st))
                if t is not True:
                    todo.append((nxt(j), later, st))
                continue
            todo.append((nxt(j), later, step(st, op, rest)))
        if verdict == "open":
            open_ended += 1
    return loads, bad, open_ended


def main():
    """the objects named, or both that hold the cooperative solvers: rdis_hip.o and refround_kernels.o (the reference-rounding
    instantiation, the one the benchmark's solve runs)"""
    objs = sys.argv[1:] or [os.path.join(ROOT, "rdis_amd", "lib", "obj", n) for n in ("rdis_hip.o", "refround_kernels.o")]
    loads, bad, open_ended = 0, [], 0
    for obj in objs:
        l, b, o = check(disassemble(obj))
        if l == 0:
            print("%s: no asynchronous granule load found" % obj)
            return 1
        loads, bad, open_ended = loads + l, bad + b, open_ended + o
    print("%d asynchronous granule loads checked, %d touched before their s_waitcnt vmcnt(0), %d reach a branch first" % (loads, len(bad), open_ended))
    for f, a, b in bad[:10]:
        print("  in %s:\n     %s\n     %s" % (f, a, b))
    return 1 if bad or loads == 0 else 0


if __name__ == "__main__":
    sys.exit(main())
