"""Compare two device-assembly listings kernel by kernel (CPU only): the check that a host-side refactor left the device code alone.

    hipcc -O3 -std=c++17 --offload-arch=gfx950 [-fno-slp-vectorize] -S --cuda-device-only unit.hip -o before.s     (at the old commit)
    ... the same at the new commit -> after.s
    python tools/asm_kernel_diff.py before.s after.s

Per kernel symbol: the instruction stream (labels renumbered per function, so the order of the kernels in the file does not matter)
and the resource block (.amdhsa_kernel ... .end_amdhsa_kernel: VGPRs, SGPRs, LDS, scratch) must be identical.  Exit status 1 otherwise.

    python tools/asm_kernel_diff.py --opcodes before.s after.s

also prints, for each kernel whose instruction stream differs, the opcodes whose counts changed: the record of a DEVICE-side refactor
(same matrix, LDS, memory, barrier and wait instructions; what moved is address arithmetic)."""
import re
import sys
from collections import Counter


def kernels(path):
    body, meta, cur, lines, mcur = {}, {}, None, [], None
    with open(path) as f:
        for l in f:
            m = re.match(r"(_Z\w+):", l)
            if m and cur is None and mcur is None:
                cur, lines = m.group(1), []
            elif cur is not None:
                if l.startswith(".Lfunc_end"):
                    body[cur], cur = lines, None
                else:
                    l = re.sub(r"\.L(BB|tmp|func_begin)\d+(_?)", r".L\1\2", l.split(";")[0]).strip()
                    if l:
                        lines.append(l)
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
            if m:
                mcur, meta[m.group(1)] = m.group(1), []
            elif mcur is not None:
                if ".end_amdhsa_kernel" in l:
                    mcur = None
                else:
                    meta[mcur].append(l.strip())
    return body, meta


def opcode_changes(x, y):
    """The opcodes whose counts differ between two instruction streams, as 'opcode before -> after' (labels and directives left out)."""
    cx, cy = (Counter(l.split()[0] for l in s if not l.endswith(":") and not l.startswith(".")) for s in (x, y))
    return [f"{op} {cx[op]} -> {cy[op]}" for op in sorted(set(cx) | set(cy)) if cx[op] != cy[op]]


def main(a, b, opcodes=False):
    (ba, ma), (bb, mb) = kernels(a), kernels(b)
    bad = 0
    for what, x, y in (("instruction stream", ba, bb), ("resource block", ma, mb)):
        for k in sorted(set(x) | set(y)):
            if k not in x or k not in y:
                print(f"{what}: {k} only in {'the second' if k not in x else 'the first'} listing")
                bad += 1
            elif x[k] != y[k]:
                print(f"{what} differs: {k}")
                bad += 1
                if opcodes and x is ba:
                    ch = opcode_changes(x[k], y[k])
                    print(f"    {len(x[k])} -> {len(y[k])} lines; " + ("; ".join(ch) if ch else "every opcode count unchanged"))
    n_inst = sum(len(v) for v in ba.values())
    print(f"{len(ba)} / {len(bb)} kernels, {len(ma)} / {len(mb)} resource blocks, {n_inst} instruction lines compared: "
          + ("identical" if not bad else f"{bad} difference(s)"))
    return 1 if bad else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--opcodes"]
    sys.exit(main(args[0], args[1], opcodes="--opcodes" in sys.argv[1:]))
