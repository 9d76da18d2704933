"""Usage: tools/isa_same.py <a.s> <b.s> - are two device listings (hipcc --cuda-device-only -S) the same code? For every function symbol, in order,
the instruction streams are compared with comments and directives stripped and the numbers of local labels (.LBB<n>_<m>, .Ltmp<n>) reduced to their order
of first appearance. Prints one line per function that differs and a summary; exit status 1 if anything differs."""
import re
import sys


def functions(path):
    out, cur, ids, text = [], None, {}, open(path).read()
    funcs = set(re.findall(r"^\s*\.type\s+([^,\s]+),@function", text, re.M))
    for line in text.split("\n"):
        line = line.split(";")[0].rstrip() if '"' not in line else line.rstrip()
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m and m.group(1) in funcs:  # a function starts
            cur, ids = [], {}
            out.append((m.group(1), cur))
            continue
        if line.startswith(".Lfunc_end"):  # ... and ends (what follows is data and metadata)
            cur = None
        s = line.strip()
        if cur is None or not s or (s.startswith(".") and not s.startswith(".L")):  # directives (.p2align, .amdhsa_*, .section ...)
            continue
        cur.append(re.sub(r"\.L(BB|tmp)\d+(_\d+)?", lambda x: ".L%d" % ids.setdefault(x.group(0), len(ids)), s))
    return out


a, b = functions(sys.argv[1]), functions(sys.argv[2])
bad = [na for (na, ba), (nb, bb) in zip(a, b) if na != nb or ba != bb]
if [n for n, _ in a] != [n for n, _ in b]:
    bad.append("the lists of function symbols (%d vs %d)" % (len(a), len(b)))
for n in bad:
    print("DIFFERS:", n)
print("%s: %d functions, %d instructions: %s" % (sys.argv[2], len(b), sum(len(x) for _, x in b), "DIFFERENT" if bad else "identical"))
sys.exit(1 if bad else 0)
