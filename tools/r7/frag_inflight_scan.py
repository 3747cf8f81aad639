"""Static check of the row kernels' in-flight LDS reads (no GPU).

gemm_phase_x3 issues its A-fragment reads by inline-asm ds_read_b128 and
retires them later by an s_waitcnt the compiler does not connect with them:
between the two, the destination registers hold stale data, and a register
copy or a spill the allocator put there would read it.  Since the first
fragment of a sub-chunk stays in flight across the next iteration's flush /
pre / DMA burst (and, at W = 512, two fragment sets are in flight), that
window holds hundreds of instructions.

This walks the disassembly of every k_step_rows instantiation in the built
library and keeps the queue of LDS / scalar-memory operations lgkmcnt counts.
An s_waitcnt lgkmcnt(N) retires all but the youngest N (LDS returns in order;
with a scalar load in the queue only lgkmcnt(0) is taken to retire anything).
Any instruction that reads or writes a VGPR of a ds_read still in the queue is
reported.  The walk is linear: it does not follow branches, so a loop's back
edge is not seen (the sub-chunk loops are fully unrolled), and it drops its
state after an unconditional branch, where the next block is reached from
elsewhere.

    python tools/r7/frag_inflight_scan.py [lib.so]      # exit 1 on a finding
"""

from __future__ import annotations

import re
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tools"))

import kernel_resources  # noqa: E402

REG = re.compile(r"\bv(\d+)\b|\bv\[(\d+):(\d+)\]")


def vregs(text: str) -> set:
    out = set()
    for m in REG.finditer(text):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
        else:
            out.update(range(int(m.group(2)), int(m.group(3)) + 1))
    return out


def scan_function(body: list) -> tuple:
    """(findings, ds_read count, longest window in instructions)."""
    queue = []          # (kind, dest vregs, issue index), oldest first
    findings, n_reads, longest = [], 0, 0
    for k, ins in enumerate(body):
        op = ins.split()[0]
        if op in ("s_branch", "s_endpgm", "s_setpc_b64"):
            queue = []      # what follows is reached from elsewhere: state unknown
            continue
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", ins)
            if m:
                n = int(m.group(1))
                if n == 0:
                    keep = []
                elif any(q[0] == "smem" for q in queue):
                    keep = queue
                else:
                    keep = queue[len(queue) - n:] if n < len(queue) else queue
                for q in queue[:len(queue) - len(keep)]:
                    longest = max(longest, k - q[2])
                queue = keep
            continue
        busy = set().union(*(q[1] for q in queue)) if queue else set()
        if busy:
            hit = vregs(ins) & busy
            # an LDS read's address operand is checked like any other use
            if hit:
                findings.append((k, ins, sorted(hit)))
        if op.startswith("ds_"):
            ops = ins[len(op):].split(",")
            dest = vregs(ops[0]) if ("read" in op or "permute" in op or "swizzle" in op
                                     or "rtn" in op) else set()
            n_reads += op.startswith("ds_read")
            queue.append(("lds", dest, k))
        elif op.startswith(("s_load", "s_buffer_load")):
            queue.append(("smem", set(), k))
    return findings, n_reads, longest


def functions(dis: str) -> dict:
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(_Z\w+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        s = re.sub(r"\s*//.*", "", line).strip()
        if name and s and not s.endswith(":"):
            out[name].append(s)
    return out


def main() -> int:
    lib = Path(sys.argv[1]) if len(sys.argv) > 1 else kernel_resources.LIB
    bad = 0
    with tempfile.TemporaryDirectory() as t:
        for co in kernel_resources.code_objects(lib, Path(t)):
            dis = subprocess.run([str(kernel_resources.LLVM / "llvm-objdump"), "-d", "--mcpu=gfx950",
                                  str(co)], capture_output=True, text=True, check=True).stdout
            for name, body in functions(dis).items():
                if "k_step_rows" not in name or "k_step_rows_ks" in name or "rows32" in name:
                    continue
                f, n, longest = scan_function(body)
                dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
                print(f"{dem}: {n} ds_read, longest in-flight window {longest} instructions, "
                      f"{len(f)} findings")
                for k, ins, hit in f[:5]:
                    print(f"    +{k}: {ins}   touches in-flight v{hit}")
                bad += len(f)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
