"""Are the kernels of two `make asm` outputs the same code?  python tools/asm_same.py OLD_DIR NEW_DIR [--renamed OLD=NEW ...]
(exit status 0: yes, 1: no)

For every kernel of OLD_DIR/*.s, NEW_DIR/*.s together must hold exactly one kernel of that demangled name whose instruction stream and
.amdhsa_* descriptor block (registers, LDS, scratch) are equal once comments and the per-file numbering of local labels are gone
(.LBB8_210 in a file with nine functions is .LBB0_210 where the function comes first).  Files of the same name in both folders are
also compared byte for byte.  Kernels that differ, are missing or occur twice are printed; kernels only NEW_DIR has are listed
and do not fail the check (a source that newly gets a listing).

--renamed OLD=NEW (any number): a kernel whose demangled name contains OLD is compared with the one kernel of NEW_DIR whose name
contains NEW instead (a template that gained an argument), each with its own symbol replaced by one token; the lines that differ are
printed, and a pair that differs in more than its `.amdhsa_kernarg_size` line is a finding."""
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


def renamed_pairs(old, new, dm, renamed):
    """Compares the renamed kernels, takes them out of `old` / `new`; returns the number of findings."""
    import difflib
    bad = 0
    for pair in renamed:
        a, b = pair.split("=", 1)
        olds, news = [n for n in old if a in dm[n]], [n for n in new if b in dm[n]]
        if len(olds) != 1 or len(news) != 1 or len(old[olds[0]]) != 1 or len(new[news[0]]) != 1:
            print(f"COUNT   --renamed {pair}: {len(olds)} kernels match in the old folder, {len(news)} in the new one")
            bad += 1
            continue
        ta, tb = old.pop(olds[0])[0][1].replace(olds[0], "KERNEL"), new.pop(news[0])[0][1].replace(news[0], "KERNEL")
        diff = [l for l in difflib.unified_diff(ta.split("\n"), tb.split("\n"), lineterm="", n=0) if not l.startswith(("---", "+++", "@@"))]
        code = [l for l in diff if ".amdhsa_kernarg_size" not in l]
        print(f"renamed {dm[olds[0]]} -> {dm[news[0]]}: {len(ta.splitlines())} lines, " + ("equal" if not diff else "differ in " + " ".join(diff)))
        bad += 1 if code else 0
    return bad


def main(old_dir, new_dir, renamed=()):
    old, new = kernels(old_dir), kernels(new_dir)
    dm = demangle(set(old) | set(new))
    n_old = len(old)
    bad_renamed = renamed_pairs(old, new, dm, renamed)
    new_by_name = {}
    for n, v in new.items():
        new_by_name.setdefault(dm[n], []).extend(v)
    bad = bad_renamed
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
    same_files, kernels_ok = 0, n_old - bad
    for path in sorted(glob.glob(os.path.join(old_dir, "*.s"))):
        other = os.path.join(new_dir, os.path.basename(path))
        if os.path.exists(other):
            if open(path, "rb").read() == open(other, "rb").read():
                same_files += 1
            elif not renamed:                        # (a renamed kernel changes its file)
                print(f"FILE    {os.path.basename(path)} is in both folders and not byte-identical")
                bad += 1
    print(f"{kernels_ok} of {n_old} kernels of {old_dir} found once and equal in {new_dir}; "
          f"{same_files} files of the same name byte-identical; {bad} findings")
    return 1 if bad else 0


if __name__ == "__main__":
    args = sys.argv[1:]
    renamed = []
    while "--renamed" in args:
        i = args.index("--renamed")
        renamed.append(args[i + 1])
        del args[i:i + 2]
    if len(args) != 2 or any("=" not in r for r in renamed):
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], renamed))
