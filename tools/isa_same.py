"""Refactoring aid: is the gfx950 device code of this tree the same as REV's?  Compiles the named translation units of
deepcharuco_amd/csrc (default dcx_conv_mfma.hip) to assembly with the Makefile's flags, once from this tree and once from
`git archive REV`, and compares kernel by kernel after dropping the __hip_cuid_ lines (a hash of the source text), the `;` comments
(`Loop: Header=BB7_5` names the kernel's position in the file) and, for the same reason, the position in local labels (.LBB7_5).  No GPU.
For a kernel that DIFFERS it also says whether every floating-point arithmetic opcode (the v_*_f64 and v_*_f32 instructions but
compares and moves) is used as often on both sides: the same counts mean rescheduled, other counts mean recomputed.  The encoding
suffixes (_e32, _e64, _dpp, _sdwa) are dropped, and v_fmac counts as v_fma: the same operation with the addend's register tied.
A kernel whose parameter list changed has another mangled name: such kernels are paired by their unmangled function name
(where that is unique on both sides) and compared like the rest.  A kernel that became a template has several instantiations of
that name here: the one whose template argument names a class of the base symbol's own parameter list is its pair
(f(RigCams, ...) with f<RigCams>).  A renamed kernel is paired by hand: --pair BASE_NAME=SUBSTRING[+SUBSTRING ...] pairs the base's
kernel of that unmangled name with the one kernel here whose symbol holds every SUBSTRING.  Where the base has several kernels of
that name (a template's instantiations), BASE_NAME+SUBSTRING[+SUBSTRING ...] names the one whose symbol holds every SUBSTRING.
usage: python tools/isa_same.py REV [--pair BASE_NAME[+SUB]=SUB[+SUB]] ... [file.hip ...]
exit status 0 only if every kernel is identical"""
import collections, os, re, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "deepcharuco_amd/csrc"
HIPCC = os.environ.get("HIPCC") or os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc")
FIGS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".private_segment_fixed_size",
        ".group_segment_fixed_size")


def git(*args):
    return subprocess.run(("git", "-C", ROOT) + args, check=True, capture_output=True, text=True).stdout.strip()


def compile_s(tree, unit, out):
    mk = open(os.path.join(tree, CSRC, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    r = subprocess.run([HIPCC] + flags + ["--cuda-device-only", "-S", os.path.join(tree, CSRC, unit), "-o", out], capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("hipcc failed on %s of %s:\n%s" % (unit, tree, r.stderr[-4000:]))
    return "".join(l for l in open(out) if "__hip_cuid_" not in l)


def fp_ops(body):
    """floating-point arithmetic opcode -> how often the body uses it"""
    n = collections.Counter()
    for l in body.split("\n"):
        m = re.match(r"\t(v_\w+)", l)
        if not m:
            continue
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1)).replace("v_fmac_", "v_fma_")
        if re.search(r"_f(64|32)$", op) and not re.match(r"v_(cmpx?|mov)_", op):
            n[op] += 1
    return n


def kernels(s):
    """name -> (function body + kernel descriptor, resource figures, instruction count, fp arithmetic opcode counts)"""
    meta = {}
    for item in re.split(r"\n  - (?=\.)", s[s.index("amdhsa.kernels:"):] if "amdhsa.kernels:" in s else ""):
        name = re.search(r"\.name:\s+(\S+)", item)
        if name:
            meta[name.group(1)] = {f: int(m.group(1)) for f in FIGS for m in [re.search(re.escape(f) + r":\s+(\d+)", item)] if m}
    res = collections.OrderedDict()
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel\n", s, re.M | re.S):
        sym = m.group(1)
        start = re.search(r"^%s:[^\n]*\n" % re.escape(sym), s, re.M).end()
        body = "\n".join(l for l in (l.split(";")[0].rstrip() for l in s[start:s.index(".Lfunc_end", start)].split("\n")) if l)
        body = re.sub(r"\.LBB\d+_", ".LBB_", body)
        n_ins = sum(1 for l in body.split("\n") if l.startswith("\t") and not l.strip().startswith((".", ";")))
        res[sym] = (body + m.group(0), meta.get(sym, {}), n_ins, fp_ops(body))
    return res


def bare_name(sym):
    """the function name inside an Itanium-mangled symbol (the last component of its nested name), or the symbol itself"""
    parts, at = [], 3 if sym.startswith("_ZN") else 2 if sym.startswith("_Z") else len(sym)
    while (m := re.compile(r"\d+").match(sym, at)):
        at = m.end() + int(m.group())
        parts.append(sym[m.end():at])
    return parts[-1] if parts else sym


def name_end(sym):
    """where the function name inside a mangled symbol ends"""
    at = sym.find(bare_name(sym))
    return len(sym) if at < 0 else at + len(bare_name(sym))


def template_classes(sym):
    """the class names in the template argument list of a mangled function symbol ([] if it is no template's instantiation)"""
    rest, names, at, depth = sym[name_end(sym):], [], 1, 0
    if not rest.startswith("I"):
        return names
    while at < len(rest):
        if (m := re.compile(r"\d+").match(rest, at)):
            at = m.end() + int(m.group())
            names.append(rest[m.end():at])
        elif (m := re.compile(r"S[0-9A-Z]*_").match(rest, at)):
            at = m.end()
        elif rest[at] == "E" and depth == 0:
            break
        else:
            depth += {"N": 1, "E": -1}.get(rest[at], 0)
            at += 1
    return names


def main():
    args, by_hand = sys.argv[1:], []
    while "--pair" in args:
        at = args.index("--pair")
        if at + 1 >= len(args) or "=" not in args[at + 1]:
            sys.exit(__doc__)
        name, subs = args[at + 1].split("=", 1)
        by_hand.append((name.split("+"), subs.split("+")))
        del args[at:at + 2]
    if not args:
        sys.exit(__doc__)
    rev, units = args[0], args[1:] or ["dcx_conv_mfma.hip"]
    dirty = git("status", "--porcelain", "--", CSRC, "include") != ""
    print("base  %s (%s)" % (git("rev-parse", rev), rev))
    print("this  %s%s" % (git("rev-parse", "HEAD"), " + working-tree changes" if dirty else ""))
    print(subprocess.run([HIPCC, "--version"], check=True, capture_output=True, text=True).stdout.split("\n")[0])
    n_same = n_all = 0
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "base")
        os.mkdir(base)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, CSRC, "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", base], input=tar, check=True)
        for unit in units:
            with ThreadPoolExecutor(2) as ex:
                fa = ex.submit(compile_s, base, unit, os.path.join(tmp, "a.s"))
                fb = ex.submit(compile_s, ROOT, unit, os.path.join(tmp, "b.s"))
                ka, kb = kernels(fa.result()), kernels(fb.result())
            print("%s: %d kernels at the base, %d here" % (unit, len(ka), len(kb)))
            # a kernel with a new parameter list or a new name: this tree's symbol is compared under the base's, if one answers
            only_a, only_b = [k for k in ka if k not in kb], [k for k in kb if k not in ka]
            for k in only_a:
                mine = [(b, h) for b, h in by_hand if b[0] == bare_name(k) and all(sub in k for sub in b[1:])]
                hand = [h for _, h in mine]
                if sum(bare_name(o) == bare_name(k) for o in only_a) != 1 and not any(len(b) > 1 for b, _ in mine):
                    continue
                if hand:
                    here = [o for o in only_b if all(sub in o for sub in hand[0])]
                else:
                    here = [o for o in only_b if bare_name(o) == bare_name(k)]
                    if len(here) > 1:
                        own = k[name_end(k):]
                        here = [o for o in here if (c := template_classes(o)) and all("%d%s" % (len(n), n) in own for n in c)]
                if len(here) == 1:
                    only_b.remove(here[0])
                    body, *rest = kb.pop(here[0])
                    kb[k] = (body.replace(here[0], k), *rest)
                    print("  paired     %s  <-  %s" % (k, here[0]))
            for sym in list(ka) + [k for k in kb if k not in ka]:
                n_all += 1
                if sym not in ka or sym not in kb:
                    print("  ONLY %s  %s" % ("base" if sym in ka else "here", sym))
                elif ka[sym][0] == kb[sym][0]:
                    n_same += 1
                    print("  identical  %s" % sym)
                else:
                    figs = "same" if ka[sym][1] == kb[sym][1] else " ".join(
                        "%s %d->%d" % (f, ka[sym][1].get(f, -1), kb[sym][1].get(f, -1)) for f in FIGS if ka[sym][1].get(f) != kb[sym][1].get(f))
                    fa, fb = ka[sym][3], kb[sym][3]
                    fp = "same" if fa == fb else " ".join("%s %d->%d" % (o, fa[o], fb[o]) for o in sorted(set(fa) | set(fb)) if fa[o] != fb[o])
                    print("  DIFFERS    %s   resource figures: %s   instructions: %d -> %d (%+d, %+.2f %%)   fp arithmetic opcode counts: %s"
                          % (sym, figs, ka[sym][2], kb[sym][2], kb[sym][2] - ka[sym][2], 100.0 * (kb[sym][2] - ka[sym][2]) / max(ka[sym][2], 1), fp))
    print("%d of %d kernels identical" % (n_same, n_all))
    sys.exit(0 if n_same == n_all and n_all > 0 else 1)


if __name__ == "__main__":
    main()
