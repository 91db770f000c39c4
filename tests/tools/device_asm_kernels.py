"""Kernel by kernel, where tests/tools/device_asm_diff.py compares file by file: a source file that GAINS kernels differs as a
whole, and a template that gains a parameter renames every instantiation.  Takes two device-assembly files (the .s files a
`device_asm_diff.py --keep <dir>` run leaves in <dir>/a and <dir>/b), cuts each into its kernels -- the instruction stream from the
kernel's label to its end, the .amdhsa_* block and the compiler's "Kernel info" comment -- rewrites the symbols of B with --rename (a
regular expression and its replacement), and compares the text kernel by kernel.  Prints `equal` / `DIFFERS` / `only in` per kernel
and a resource line for each kernel of B; exits non-zero when a kernel both files hold differs.  Needs no GPU.

    python tests/tools/device_asm_kernels.py <dir>/a/meme_challenge_amd/csrc/optim.hip.s <dir>/b/meme_challenge_amd/csrc/optim.hip.s \\
        --rename 'adam_kernelILi(\\d)ELb(\\d)ELb0EEEvNS_8WalkArgsIXT0_EXT1_EEE' 'adam_kernelILi\\1ELb\\2EEEvNS_8WalkArgsIXT0_EEE'"""
import argparse
import re
import subprocess
import sys


def kernels(path, rename):
    """name -> the lines that belong to the kernel (symbols rewritten), in file order"""
    with open(path) as f:
        text = f.read()
    if rename:
        text = re.sub(rename[0], rename[1], text)
    lines = [l for l in text.splitlines() if '__hip_cuid_' not in l]
    names = [m.group(1) for l in lines for m in [re.match(r'\s*\.amdhsa_kernel\s+(\S+)', l)] if m]
    # labels carry the function's NUMBER in the file (.LBB7_4, .Lfunc_end7, "Header=BB7_6"): a new kernel in front renumbers the
    # rest, and a longer number shifts the column of the comment behind it
    norm = lambda l: re.sub(r'\s+;', ' ;', re.sub(r'(BB|func_begin|func_end|tmp)\d+', r'\1N', l))
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ':'))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith('; Occupancy:'))      # closes the "Kernel info" comment
        out[name] = [norm(l) for l in lines[start:end + 1]]
    return out


def resources(body):
    get = lambda key: next((l.split()[-1] for l in body if re.match(r'\s*(;\s*)?' + re.escape(key), l)), '?')
    return 'VGPRs %s  SGPRs %s  LDS %s B  scratch %s B  occupancy %s waves/SIMD  %d instructions' % (
        get('.amdhsa_next_free_vgpr'), get('.amdhsa_next_free_sgpr'), get('.amdhsa_group_segment_fixed_size'),
        get('.amdhsa_private_segment_fixed_size'), get('Occupancy:'),
        sum(1 for l in body if re.match(r'\t[a-z]+_[a-z0-9_]+', l) and not l.lstrip().startswith('.')))


def demangle(name):
    try:
        return subprocess.run(['c++filt', name], capture_output=True, text=True).stdout.strip() or name
    except OSError:
        return name


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('asm_a')
    ap.add_argument('asm_b')
    ap.add_argument('--rename', nargs=2, metavar=('REGEX', 'REPL'), help='rewrite the symbols of B before comparing')
    args = ap.parse_args()
    a, b = kernels(args.asm_a, None), kernels(args.asm_b, args.rename)
    differing = 0
    for name in list(a) + [n for n in b if n not in a]:
        if name not in a or name not in b:
            print('%-10s %s' % ('only in ' + ('A' if name in a else 'B'), demangle(name)))
        elif a[name] == b[name]:
            print('%-10s %s (%d lines)' % ('equal', demangle(name), len(a[name])))
        else:
            differing += 1
            i = next((k for k, (x, y) in enumerate(zip(a[name], b[name])) if x != y), min(len(a[name]), len(b[name])))
            print('%-10s %s from line %d of the kernel (%d / %d lines)' % ('DIFFERS', demangle(name), i + 1, len(a[name]), len(b[name])))
            for tag, ls in (('A', a[name]), ('B', b[name])):
                for l in ls[i:i + 3]:
                    print('    %s: %s' % (tag, l))
    print('resources of B:')
    for name, body in b.items():
        print('  %s\n      %s' % (demangle(name), resources(body)))
    print('%d kernels differ' % differing)
    sys.exit(1 if differing else 0)


if __name__ == '__main__':
    main()
