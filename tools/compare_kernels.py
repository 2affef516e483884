"""Are the kernels of two trees the same machine code?  For a refactor that must not change code generation.

    python tools/compare_kernels.py --build TREE OUT     device code of TREE's ppca_rs_amd/csrc/*.hip -> OUT/<name>.elf (gfx950,
                                                         the flags of ppca_rs_amd/build.py; needs no GPU)
    python tools/compare_kernels.py OLD NEW              compares two such directories, file by file
    python tools/compare_kernels.py --pooled [--namespace OLD=NEW] [--rename OLDSYM=NEWSYM]... OLD NEW
                                                         follows kernels that moved to another file or namespace (below)

Per kernel symbol: the bytes of its function in .text with the disassembly's own addresses left out (a function that moved is
still the same function), and .vgpr_count / .sgpr_count / .group_segment_fixed_size / .private_segment_fixed_size of its metadata
note.  Prints one line per file and every kernel that differs, appeared or disappeared; exits 1 when a kernel present on both
sides differs or one appeared (kernels that disappeared are listed: whether they were meant to go is the reader's call).
Whole files are not compared: two builds of identical code differ in a few bytes outside the sections.

One kind of operand depends on where the function lies and is compared as equal: the 32-bit literal of the s_add_u32 / s_addc_u32
pair that follows an s_getpc_b64 on the same register pair -- the distance from the code to a constant table in another section
(lean_log's coefficients, for one).  Deleting a kernel from a file moves the others and changes nothing else in them.  The line
of a file says how many such literals were masked on either side.  The zero padding between a function and the next is left out too.

--pooled: the kernels of all .elf files of a side are one pool, and a kernel's partner is the one of the same mangled name wherever
it lies.  --namespace 12_GLOBAL__N_1=7ppca_sp rewrites that component of OLD's names textually (a file's anonymous namespace that
became the named namespace ppca_sp; length-prefixed as in the mangled name, so no demangler is needed; a kernel whose unchanged name
exists in NEW keeps it, as in a file that was not touched); --rename gives a partner by hand, to a kernel that became an instantiation
of a template for one.  A kernel's own name shows in its disassembly, in the
`<symbol+0x...>` comment behind each branch: that comment is dropped before the comparison, as is the s_nop / s_code_end padding
behind the last instruction.  The exit status is as above; a kernel of NEW without a partner counts as one that appeared.
"""
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
LLVM = os.path.join(ROCM, "lib", "llvm", "bin")
META = (".vgpr_count", ".sgpr_count", ".group_segment_fixed_size", ".private_segment_fixed_size")


def build(tree, out):
    csrc = os.path.join(tree, "ppca_rs_amd", "csrc")
    os.makedirs(out, exist_ok=True)

    def one(src):
        base = os.path.join(out, src[:-4])
        subprocess.check_call([os.path.join(ROCM, "bin", "hipcc"), "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only",
                               "-c", os.path.join(csrc, src), "-o", base + ".co"])
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + base + ".co",
                               "--targets=hip-amdgcn-amd-amdhsa--gfx950", "--output=" + base + ".elf"])
        os.remove(base + ".co")

    srcs = sorted(f for f in os.listdir(csrc) if f.endswith(".hip") and f not in ("ppca_capi.hip", "ppca_comm.hip"))  # (host only)
    with ThreadPoolExecutor(max_workers=min(len(srcs), os.cpu_count() or 1)) as ex:
        list(ex.map(one, srcs))


def mask_pcrel(lines):
    """The literal (operand and encoding dword) of the s_add_u32 lo / s_addc_u32 hi behind `s_getpc_b64 s[lo:hi]` -> <pcrel>; how many."""
    n, want = 0, []  # want: the registers whose additions are still expected, in order
    for i, ln in enumerate(lines):
        m = re.match(r"\s*s_getpc_b64 s\[(\d+):(\d+)\]", ln)
        if m:
            want = [("s_add_u32", m.group(1)), ("s_addc_u32", m.group(2))]
            continue
        if want:
            op, reg = want.pop(0)
            m = re.match(r"(\s*%s s%s, s%s, )\S+(\s+// [0-9A-F]{8}) [0-9A-F]{8}$" % (op, reg, reg), ln)
            if m:
                lines[i] = m.group(1) + "<pcrel>" + m.group(2) + " <pcrel>"
                n += 1
            else:
                want = []
    return n


def kernels(elf):
    """{kernel symbol: (code without addresses and position-dependent literals, metadata tuple)}, literals masked"""
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", elf], check=True, capture_output=True, text=True).stdout
    meta = {}
    for blk in re.split(r"\n\s*- \.agpr_count:|\n\s*- \.args:", notes)[1:]:
        sym = re.search(r"\.symbol:\s+'?([^\s']+?)\.kd'?\s", blk)
        if sym:
            meta[sym.group(1)] = tuple(int(re.search(re.escape(k) + r":\s+(\d+)", blk).group(1)) for k in META)
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-leading-addr", elf], check=True, capture_output=True, text=True).stdout
    code, cur = {}, None
    for ln in dis.split("\n"):
        m = re.match(r"<(\S+)>:$", ln)
        if m:
            cur = m.group(1)
            code[cur] = []
        elif cur is not None and ln.strip():
            code[cur].append(re.sub(r"\s*//\s*[0-9A-Fa-f]+:", " //", ln))  # the trailing "// address: encoding" keeps the encoding
    for lines in code.values():  # (zero padding up to the next function's alignment, printed as "...": depends on the neighbour)
        while lines and lines[-1].strip() == "...":
            lines.pop()
    masked = sum(mask_pcrel(code.get(k, [])) for k in meta)
    return {k: ("\n".join(code.get(k, [])), v) for k, v in meta.items()}, masked


def main(old, new):
    bad = 0
    for f in sorted(set(os.listdir(old)) | set(os.listdir(new))):
        if not f.endswith(".elf"):
            continue
        if not os.path.exists(os.path.join(new, f)):
            print("%-22s only in OLD (%d kernels)" % (f, len(kernels(os.path.join(old, f))[0])))
            continue
        if not os.path.exists(os.path.join(old, f)):
            print("%-22s only in NEW" % f)
            bad += 1
            continue
        (a, ma), (b, mb) = kernels(os.path.join(old, f)), kernels(os.path.join(new, f))
        both = sorted(set(a) & set(b))
        diff = [k for k in both if a[k] != b[k]]
        gone, came = sorted(set(a) - set(b)), sorted(set(b) - set(a))
        print("%-22s old %3d  new %3d  identical %3d  differ %d  gone %d  new-only %d  pc-relative literals masked %d / %d"
              % (f, len(a), len(b), len(both) - len(diff), len(diff), len(gone), len(came), ma, mb))
        for k in diff:
            print("   DIFFERS  %s  %s meta %s -> %s" % (k, "code" if a[k][0] != b[k][0] else "", a[k][1], b[k][1]))
        for k in gone:
            print("   gone     %s" % k)
        for k in came:
            print("   NEW      %s" % k)
        bad += len(diff) + len(came)
    return 1 if bad else 0


def pool(d):
    """{kernel symbol: (normalised code, metadata, file)} over the .elf files of d"""
    out = {}
    for f in sorted(os.listdir(d)):
        if f.endswith(".elf"):
            for k, (code, meta) in kernels(os.path.join(d, f))[0].items():
                lines = [re.sub(r"\s*<[^<>\s]+>$", "", ln) for ln in code.split("\n")]
                while lines and re.match(r"\s*(s_nop|s_code_end)\b", lines[-1]):
                    lines.pop()
                if k in out:
                    sys.exit("%s: %s is also a kernel of %s: the pool cannot tell them apart" % (f, k, out[k][2]))
                out[k] = ("\n".join(lines), meta, f)
    return out


def main_pooled(old, new, namespaces, renames):
    a, b = pool(old), pool(new)
    partner = {}  # OLD symbol -> the name it should have in NEW
    for k in a:
        name = k
        for frm, to in namespaces:
            name = name.replace(frm, to)
        partner[k] = renames.get(k, k if k in b else name)  # (a file that did not change keeps its anonymous namespace)
    bad = 0
    for f in sorted(set(v[2] for v in a.values())):
        mine = sorted(k for k in a if a[k][2] == f)
        found = [k for k in mine if partner[k] in b]
        diff = [k for k in found if a[k][:2] != b[partner[k]][:2]]
        where = {}
        for k in found:
            where[b[partner[k]][2]] = where.get(b[partner[k]][2], 0) + 1
        print("%-22s old %3d  matched %3d  identical %3d  differ %d  gone %d   now in: %s"
              % (f, len(mine), len(found), len(found) - len(diff), len(diff), len(mine) - len(found),
                 ", ".join("%s %d" % kv for kv in sorted(where.items()))))
        for k in diff:
            print("   DIFFERS  %s -> %s (%s)  %s meta %s -> %s" % (k, partner[k], b[partner[k]][2], "code" if a[k][0] != b[partner[k]][0] else "",
                                                               a[k][1], b[partner[k]][1]))
        for k in mine:
            if k not in found:
                print("   gone     %s" % k)
        bad += len(diff)
    came = sorted(set(b) - set(partner.values()))
    for k in came:
        print("   NEW      %s (%s)" % (k, b[k][2]))
    print("total: old %d  new %d  matched %d  differ %d  without a partner in OLD %d" % (len(a), len(b), len(set(partner.values()) & set(b)), bad, len(came)))
    return 1 if bad or came else 0


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--build":
        build(sys.argv[2], sys.argv[3])
    elif len(sys.argv) >= 4 and sys.argv[1] == "--pooled":
        args, namespaces, renames = sys.argv[2:], [], {}
        while len(args) > 2 and args[0] in ("--namespace", "--rename"):
            frm, to = args[1].split("=", 1)
            if args[0] == "--namespace":
                namespaces.append((frm, to))
            else:
                renames[frm] = to
            args = args[2:]
        if len(args) != 2:
            sys.exit(__doc__)
        sys.exit(main_pooled(args[0], args[1], namespaces, renames))
    elif len(sys.argv) == 3:
        sys.exit(main(sys.argv[1], sys.argv[2]))
    else:
        sys.exit(__doc__)
