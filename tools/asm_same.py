"""Are the kernels of two `make asm` outputs the same code?  python tools/asm_same.py OLD_DIR NEW_DIR  (exit status 0: yes, 1: no)

For every kernel of OLD_DIR/*.s, NEW_DIR/*.s together must hold exactly one kernel of that demangled name whose instruction stream and
.amdhsa_* descriptor block (registers, LDS, scratch) are equal once comments and the per-file numbering of local labels are gone
(.LBB8_210 in a file with nine functions is .LBB0_210 where the function comes first).  Files of the same name in both folders are
also compared byte for byte.  Kernels that differ, are missing or occur twice are printed; kernels only NEW_DIR has are listed
and do not fail the check (a source that newly gets a listing)."""
import glob, os, re, subprocess, sys


def kernels(folder):
    """{mangled name: [(file, normalised text from the entry label to .Lfunc_end, descriptor block included)]}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, "*.s"))):
        lines = open(path).read().split("\n")
        for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", "\n".join(lines), re.M):
            i = lines.index(next(l for l in lines if l.startswith(name + ":")))
            body = []
            for l in lines[i + 1:]:
                l = re.sub(r"\.L([A-Za-z_]+?)\d+(?=_\d|\b)", r".L\1", l.split(";")[0]).strip()
                if re.match(r"\.Lfunc_end:", l):
                    break
                if l:
                    body.append(l)
            out.setdefault(name, []).append((os.path.basename(path), "\n".join(body)))
    return out


def demangle(names):
    names = list(names)
    try:
        return dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main(old_dir, new_dir):
    old, new = kernels(old_dir), kernels(new_dir)
    dm = demangle(set(old) | set(new))
    new_by_name = {}
    for n, v in new.items():
        new_by_name.setdefault(dm[n], []).extend(v)
    bad = 0
    for n in sorted(old, key=dm.get):
        (f_old, text), hits = old[n][0], new_by_name.pop(dm[n], [])
        if len(old[n]) != 1 or len(hits) != 1:
            print(f"COUNT   {dm[n]}: {len(old[n])} in {old_dir}, {len(hits)} in {new_dir}")
        elif hits[0][1] != text:
            a, b = text.split("\n"), hits[0][1].split("\n")
            first = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            print(f"DIFFERS {dm[n]}: {f_old} {len(a)} lines, {hits[0][0]} {len(b)} lines, first difference at line {first} of the kernel")
        else:
            continue
        bad += 1
    for name, hits in sorted(new_by_name.items()):
        print(f"new     {name} ({hits[0][0]})")
    same_files, kernels_ok = 0, len(old) - bad
    for path in sorted(glob.glob(os.path.join(old_dir, "*.s"))):
        other = os.path.join(new_dir, os.path.basename(path))
        if os.path.exists(other):
            if open(path, "rb").read() == open(other, "rb").read():
                same_files += 1
            else:
                print(f"FILE    {os.path.basename(path)} is in both folders and not byte-identical")
                bad += 1
    print(f"{kernels_ok} of {len(old)} kernels of {old_dir} found once and equal in {new_dir}; "
          f"{same_files} files of the same name byte-identical; {bad} findings")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
