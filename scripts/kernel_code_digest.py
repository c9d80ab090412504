"""The device code two builds of the package hold, kernel by kernel, for showing that a change left every kernel's machine code alone.

    python3 scripts/kernel_code_digest.py ROOT_A ROOT_B [NAME_REGEX] [> FILE]   # each ROOT: the root of a built tree (gbrl_amd/libgbrl_hip.so inside it)

Needs no GPU.  Every gfx950 code object of each library's fat binary is taken out, disassembled with llvm-objdump and its notes read with
llvm-readelf.  Per kernel symbol: the sha256 of its instruction text (mnemonics and operands; addresses and encodings dropped, so that the place
of a kernel inside its code object does not count) and the kernel-descriptor figures -- VGPRs, SGPRs, LDS bytes, scratch bytes, kernarg bytes.
A line per kernel (with NAME_REGEX: per kernel whose name it matches, and per kernel that is not the same on both sides), then the counts over ALL
kernels: only in A, only in B, differing.  Exit status 1 unless all three are 0.  (A name that several
translation units define -- a template both instantiate -- counts once per definition, the definitions ordered by their hash.)
"""
import hashlib
import os
import re
import struct
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIGURES = (("vgpr", ".vgpr_count"), ("sgpr", ".sgpr_count"), ("lds", ".group_segment_fixed_size"), ("scratch", ".private_segment_fixed_size"),
           ("kernarg", ".kernarg_segment_size"))


def code_objects(lib):
    """the gfx950 code objects of every offload bundle in the library (uncompressed bundles: header, then the entries' images)"""
    data = open(lib, "rb").read()
    pos = data.find(MAGIC)
    while pos >= 0:
        (n,) = struct.unpack_from("<Q", data, pos + len(MAGIC))
        at = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", data, at)
            triple = data[at + 24:at + 24 + tlen].decode()
            at += 24 + tlen
            if "gfx950" in triple and size:
                yield data[pos + off:pos + off + size]
        pos = data.find(MAGIC, pos + len(MAGIC))


def kernels_of(image, tmp):
    path = os.path.join(tmp, "co.elf")
    with open(path, "wb") as f:
        f.write(image)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", path], capture_output=True, text=True, check=True).stdout
    figures, items = {}, []
    for line in notes.splitlines():          # the metadata is YAML: an item of amdhsa.kernels opens with "  - .key:", its own keys sit at four spaces
        m = re.match(r"^  ([- ]) (\.\w+):\s*(\S+)\s*$", line)
        if m:
            if m.group(1) == "-":
                items.append({})
            items[-1][m.group(2)] = m.group(3).strip("'\"")
    for item in items:
        if ".name" in item:
            figures[item[".name"]] = {short: item.get(key, "?") for short, key in FIGURES}
    # a kernel's text ends where its symbol does: what follows it (alignment padding, the end-of-code filler behind a unit's last kernel) is not its code
    end = {}
    for line in subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", path], capture_output=True, text=True, check=True).stdout.splitlines():
        f = line.split()
        if len(f) == 8 and f[3] == "FUNC" and f[7] in figures:
            end[f[7]] = int(f[1], 16) + int(f[2])
    asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", path], capture_output=True, text=True, check=True).stdout
    out, cur = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = m.group(1) if m.group(1) in end else None
            if cur:
                out[cur] = []
            continue
        m = re.match(r"^\s+(\S.*?)\s*// ([0-9A-F]+):", line)
        if cur and m and int(m.group(2), 16) < end[cur]:
            out[cur].append(" ".join(m.group(1).split()))
    return [(k, hashlib.sha256("\n".join(v).encode()).hexdigest()[:16], len(v), figures[k]) for k, v in out.items()]


def digest(root):
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for image in code_objects(os.path.join(root, "gbrl_amd", "libgbrl_hip.so")):
            for name, sha, n, fig in kernels_of(image, tmp):
                table.setdefault(name, []).append("%s insns=%d %s" % (sha, n, " ".join("%s=%s" % (s, fig.get(s, "?")) for s, _ in FIGURES)))
    return {(name, i): d for name, ds in table.items() for i, d in enumerate(sorted(ds))}


def main(root_a, root_b, shown=""):
    a, b = digest(root_a), digest(root_b)
    only_a, only_b, differ = [], [], []
    for key in sorted(set(a) | set(b)):
        name = key[0] + ("#%d" % key[1] if key[1] else "")
        if key not in b:
            only_a.append(name)
            print("ONLY-A %s  %s" % (name, a[key]))
        elif key not in a:
            only_b.append(name)
            print("ONLY-B %s  %s" % (name, b[key]))
        elif a[key] != b[key]:
            differ.append(name)
            print("DIFFER %s  A: %s  B: %s" % (name, a[key], b[key]))
        elif re.search(shown, key[0]):
            print("same   %s  A = B: %s" % (name, a[key]))
    print("# kernels: A %d, B %d; only in A %d, only in B %d, differing %d" % (len(a), len(b), len(only_a), len(only_b), len(differ)))
    return 1 if only_a or only_b or differ else 0


if __name__ == "__main__":
    if len(sys.argv) not in (3, 4):
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
