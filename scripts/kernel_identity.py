"""Are the kernels of two device assembly files (what `make asm` writes, build/rt_kernels.s) the same code? Per kernel:
the text from its symbol to its .Lfunc_end label (the instructions and the .amdhsa_kernel ... .end_amdhsa_kernel block),
with `;` comments and blank lines dropped and the function-numbered local labels (.LBB<k>_, .Lfunc_end<k>, .LJTI<k>_)
renumbered to one token, so the order in which the compiler emits the kernels does not count; neither does the
per-compilation __hip_cuid_<hash> symbol. Compares only; exit status 1 when a kernel differs or exists on one side only.

usage: python scripts/kernel_identity.py OLD.s NEW.s > profiles/rNN/kernel_identity.txt
"""
import re
import sys
from pathlib import Path

LOCAL = re.compile(r"\.(LBB|Lfunc_end|LJTI)\d+")


def kernels(path: str) -> dict:
    lines = Path(path).read_text().splitlines()
    names = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln) for ln in lines) if m}
    out, cur = {}, None
    for ln in lines:
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
        if m and m.group(1) in names:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None:
            continue
        code = re.sub(r"__hip_cuid_[0-9a-f]+", "__hip_cuid", LOCAL.sub(r".\1", ln.split(";")[0])).strip()
        if code:
            cur.append(code)
        if code.startswith(".Lfunc_end"):
            cur = None
    assert set(out) == names, "a kernel descriptor without a function body"
    return out


def main() -> int:
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    print(f"kernels: {len(old)} old, {len(new)} new; {len(differ)} differ, {len(only_old)} only old, {len(only_new)} only new")
    for tag, ks in (("differs", differ), ("only old", only_old), ("only new", only_new)):
        for k in ks:
            print(f"{tag}: {k}")
    return 1 if differ or only_old or only_new else 0


if __name__ == "__main__":
    sys.exit(main())
