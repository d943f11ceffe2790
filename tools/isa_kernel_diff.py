"""Which kernels of two gfx950 ISA listings of one source (hipcc -S --cuda-device-only) differ: per kernel, the instruction text from its
label to s_endpgm with block labels renumbered, compared line by line.  Trailing zero / false template arguments are cut from the
mangled names (ILi96ELi96ELb0ELi0EE -> ILi96ELi96EE) so that a kernel that only gained defaulted parameters still finds its parent.
    python tools/isa_kernel_diff.py parent.s new.s"""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    for ln in open(path):
        m = re.match(r"^(_Z\w+):", ln)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            code = ln.split(";")[0].rstrip()
            if code.strip():
                body.append(re.sub(r"\.LBB\d+_", ".LBB_", code))
            if "s_endpgm" in ln:
                out[re.sub(r"(ELi0)+EE", "EE", name.replace("ELb", "ELi"))] = body
                name = None
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print("%-100s only in the %s listing (%d instructions)" % (k, "second" if k in b else "first", len((b if k in b else a)[k])))
        else:
            print("%-100s %s (%d instructions)" % (k, "identical" if a[k] == b[k] else "DIFFERENT (%d before)" % len(a[k]), len(b[k])))


if __name__ == "__main__":
    main()
