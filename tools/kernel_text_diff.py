"""Do two source trees compile to the same kernels?  The check behind "the parent's bits" in a kernel commit, without a GPU.

    python tools/kernel_text_diff.py [--pair OLD=NEW ...] TREE_A TREE_B file.hip [file.hip:MACRO=VALUE ...]

Each file (a path inside the tree, or a bare name under tf-mpc_amd/csrc) is compiled in both trees to device assembly with
check_ring_waits.FLAGS --cuda-device-only -S; `file.hip:MACRO=VALUE` adds -DMACRO=VALUE (ilqr_adjoint_mfma.hip:TFMPC_AM_PART=3).
Kernels are paired by demangled name without the parameter list, so a renamed argument type still pairs (without llvm-cxxfilt or
c++filt: by mangled name, and such a kernel is reported as unpaired).  A kernel that was renamed on purpose is paired by hand:
--pair OLD=NEW (repeatable; each side a substring of one demangled name, OLD in tree A, NEW in tree B).  Per kernel it compares
  * the instruction text between the kernel's label and its .amdhsa_kernel line: comments and directives stripped, block labels
    kept, the function index in .LBB<i>_<k> and the names of kernels and of the __hip_cuid_* symbol normalised;
  * .amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr and .amdhsa_private_segment_fixed_size;
and prints one line: identical, or the first differing instruction / count.  Exit status 1 if anything differs or is unpaired."""
import os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from check_ring_waits import FLAGS, hipcc_path  # noqa: E402

COUNTS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size")


def assembly(tree, spec, tmp):
    name, _, macro = spec.partition(":")
    src = os.path.join(tree, name)
    if not os.path.exists(src):
        src = os.path.join(tree, "tf-mpc_amd", "csrc", name)
    out = tempfile.mkstemp(suffix=".s", dir=tmp)[1]
    subprocess.run([hipcc_path(), *FLAGS, *([f"-D{macro}"] if macro else []), "--cuda-device-only", "-S", src, "-o", out], check=True,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return open(out).read()


def demangled(names):
    tool = next((t for t in (os.path.join(os.path.dirname(os.path.realpath(hipcc_path())), "..", "llvm", "bin", "llvm-cxxfilt"),
                             shutil.which("llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if tool is None or not names:
        return list(names)
    return subprocess.run([tool, *names], check=True, capture_output=True, text=True).stdout.split("\n")[:len(names)]


def key_of(text):
    """demangled name without its trailing parameter list and without a leading return type"""
    if text.endswith(")"):
        depth = 0
        for i in range(len(text) - 1, -1, -1):
            depth += (text[i] == ")") - (text[i] == "(")
            if depth == 0:
                text = text[:i]
                break
    return re.sub(r"^void ", "", text)


def kernels(text):
    """key -> (instruction lines, {count name: value})"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, flags=re.M)
    keys = dict(zip(names, (key_of(d) for d in demangled(names))))
    any_kernel = re.compile("|".join(sorted(map(re.escape, names), key=len, reverse=True)) or r"$^")
    out = {}
    for name in names:
        m = re.search(r"^" + re.escape(name) + r":.*?\n(.*?)^\s*\.amdhsa_kernel\s+" + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", text,
                      flags=re.S | re.M)
        lines = []
        for line in m.group(1).split("\n"):
            s = line.split(";")[0].strip()
            if not s or ((s.startswith(".") or s.endswith(":")) and not re.match(r"^\.LBB\d+_\d+:$", s)):
                continue                                   # blank, a directive, or a label that is not a basic block's
            s = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", s)
            s = any_kernel.sub("<kernel>", s)
            lines.append(re.sub(r"__hip_cuid_\w+", "__hip_cuid", re.sub(r"\s+", " ", s)))
        counts = {c: int(re.search(r"\.amdhsa_" + c + r"\s+(\d+)", m.group(2)).group(1)) for c in COUNTS}
        key, i = keys[name], 1
        while key in out:                                  # overloads that differ in their parameters only
            i += 1
            key = f"{keys[name]} #{i}"
        out[key] = (lines, counts)
    return out


def compare(a, b, pairs=()):
    """(kernels compared, list of findings) for the two assembly texts of one file"""
    ka, kb = kernels(a), kernels(b)
    for old, new in pairs:                                 # a renamed kernel takes its old key, where both sides name exactly one
        src, dst = [k for k in ka if old in k], [k for k in kb if new in k]
        if len(src) == len(dst) == 1:
            kb[src[0]] = kb.pop(dst[0])
    bad = 0
    for key in list(ka) + [k for k in kb if k not in ka]:
        if key not in ka or key not in kb:
            print(f"  UNPAIRED   {key}: only in tree {'A' if key in ka else 'B'}")
            bad += 1
            continue
        (la, ca), (lb, cb) = ka[key], kb[key]
        first = next((i for i, (x, y) in enumerate(zip(la, lb)) if x != y), None if len(la) == len(lb) else min(len(la), len(lb)))
        if first is not None:
            x, y = (l[first] if first < len(l) else "<end>" for l in (la, lb))
            print(f"  DIFFERENT  {key}: line {first} of {len(la)} / {len(lb)}: `{x}` | `{y}`")
        elif ca != cb:
            print(f"  DIFFERENT  {key}: same {len(la)} lines, counts {ca} | {cb}")
        else:
            print(f"  identical  {key}: {len(la)} lines, vgpr {ca[COUNTS[0]]}, sgpr {ca[COUNTS[1]]}, private {ca[COUNTS[2]]}")
        bad += first is not None or ca != cb
    return len(set(ka) | set(kb)), bad


if __name__ == "__main__":
    argv, pairs = sys.argv[1:], []
    while "--pair" in argv[:-1]:
        i = argv.index("--pair")
        pairs.append(tuple(argv[i + 1].split("=", 1)))
        del argv[i:i + 2]
    if len(argv) < 3 or any(len(p) != 2 for p in pairs):
        sys.exit(__doc__)
    tree_a, tree_b, specs = argv[0], argv[1], argv[2:]
    total = bad = 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        jobs = [(spec, pool.submit(assembly, tree_a, spec, tmp), pool.submit(assembly, tree_b, spec, tmp)) for spec in specs]
        for spec, fa, fb in jobs:
            print(spec)
            n, b = compare(fa.result(), fb.result(), pairs)
            total += n
            bad += b
    print(f"{total} kernels in {len(specs)} translation units: {total - bad} identical, {bad} different or unpaired")
    sys.exit(1 if bad else 0)
