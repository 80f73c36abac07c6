#!/usr/bin/env python3
"""Compare the step kernels of two builds instantiation by instantiation (no GPU needed).

For each of the four step translation units compile both trees with the flags of smplsim_amd/_lib.py plus
`--cuda-device-only -S -Rpass-analysis=kernel-resource-usage`, assembly to DIR/<unit>.s and the remarks (stderr) to
DIR/<unit>.remarks; then

    python tools/step_kernel_asm_diff.py PARENT_DIR CHANGE_DIR

prints, per ss_env_kernel instantiation, VGPRs / scratch bytes per lane / occupancy of both builds and whether the kernel's code
(its label to the end of the function: instructions and kernel descriptor; the compiler's comments and local label numbers
removed) is identical apart from what follows from the size of the kernel arguments.  Instantiations are matched by their
template arguments; those that only the change has are listed with their resources.  The optional-I/O instantiations (the trailing
CFORCE switch: contact-force output, body-wrench input) are where optional features are compiled in: a change to them is reported with
both builds' resources and is not a violation — the rule is for the kernels that run with every option off.
"""
import re
import subprocess
import sys

UNITS = ("smplsim_hip", "smplsim_hip_sc", "smplsim_hip_im", "smplsim_hip_x")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def bodies(path):
    """{mangled kernel name: normalised instruction lines}"""
    out, name, cur = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w*ss_env_kernel\w*):", line)
        if m:
            name, cur = m.group(1), []
            continue
        if name is None:
            continue
        s = line.split(";")[0].rstrip()
        if s.strip().startswith(".Lfunc_end"):
            out[name] = cur
            name = None
            continue
        if not s.strip() or s.strip().startswith((".p2align", ".loc", ".cfi", ".file")):
            continue
        cur.append(re.sub(r"\.L(BB|tmp|func_begin|func_end|post_getpc)\d+_?\d*", ".L", s))
    return out


def resources(path):
    """{mangled kernel name: (VGPRs, scratch bytes per lane, occupancy)}"""
    out, name, cur = {}, None, {}
    for line in open(path):
        m = re.search(r"remark: +(Function Name|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]): (\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            name, cur = m.group(2), {}
            out[name] = cur
        elif name:
            cur[m.group(1).split()[0]] = int(m.group(2))
    return {k: (v.get("VGPRs"), v.get("ScratchSize"), v.get("Occupancy")) for k, v in out.items()}


def keyed(names):
    """{(template arguments without the trailing CFORCE switch, CFORCE): mangled name}; the parent's kernels have no such switch"""
    if not names:
        return {}
    out = {}
    for mangled, d in demangle(sorted(names)).items():
        args = re.sub(r"ss::HdrFixedT<(\d+),[^>]*>", r"Fixed\1", d)
        args = re.search(r"ss_env_kernel<(.*)>\(", args).group(1).replace("ss::HdrRuntime", "Runtime").split(", ")
        out[(", ".join(args[:10]), len(args) > 10 and args[10] == "true")] = mangled
    return out


def same_code(a, b, name_a, name_b):
    """Code equal apart from what follows from sizeof(KArgs): .amdhsa_kernarg_size and the offsets of the implicit arguments, which
    lie behind the explicit ones (the last 256 bytes of the kernel arguments), where the kernel reads them or forms their address."""
    size = lambda body: next(int(l.split()[-1]) for l in body if ".amdhsa_kernarg_size" in l)
    def norm(body, name):                                   # (the change's kernels carry one more template argument in their names)
        end = size(body) - 256
        rel = lambda m: "KARGS_END+%d" % (int(m.group(0), 16) - end) if end <= int(m.group(0), 16) < end + 256 else m.group(0)
        return [(re.sub(r"0x[0-9a-f]+", rel, l) if l.strip().startswith(("s_add_u32", "s_load")) else l).replace(name, "KERNEL")
                for l in body if ".amdhsa_kernarg_size" not in l]
    return norm(a, name_a) == norm(b, name_b)


def main(parent, change):
    worse = 0
    hdr = f"{'instantiation <DOFP,CANDP,SLOTP,NPASS,threads,BODYOUT,SHAPED,header,SELFCOL,IMIT>':66s} {'VGPRs':>9s} {'scratch B':>11s} {'occupancy':>9s}  instructions"
    for u in UNITS:
        bp, bc = bodies(f"{parent}/{u}.s"), bodies(f"{change}/{u}.s")
        rp, rc = resources(f"{parent}/{u}.remarks"), resources(f"{change}/{u}.remarks")
        kp, kc = keyed(bp), keyed(bc)
        print(f"== {u}.hip   (parent/change)")
        print(hdr)
        for key in sorted(kp):
            n0, n1 = kp[key], kc[key]
            same = same_code(bp[n0], bc[n1], n0, n1)
            (v0, s0, o0), (v1, s1, o1) = rp[n0], rc[n1]
            bad = (not same or s1 > s0) and not key[1]
            worse += bad
            print(f"{key[0] + (', CFORCE' if key[1] else ''):66s} {v0:4d}/{v1:<4d} {s0:5d}/{s1:<5d} {o0:4d}/{o1:<4d}  {'identical' if same else 'differ'} ({len(bp[n0])}/{len(bc[n1])}){'  <-- NOT ACCEPTED' if bad else ''}")
        for key in sorted(k for k in kc if k not in kp):
            v1, s1, o1 = rc[kc[key]]
            print(f"{key[0] + (', CFORCE' if key[1] else ''):66s} {'-':>4s}/{v1:<4d} {'-':>5s}/{s1:<5d} {'-':>4s}/{o1:<4d}  new ({len(bc[kc[key]])})")
    print("every kernel of the parent without the optional I/O must be identical apart from the kernel-argument size, and its scratch must not grow:", "OK" if not worse else f"{worse} VIOLATIONS")
    return 1 if worse else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:3]))
