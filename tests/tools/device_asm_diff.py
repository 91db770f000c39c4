"""Did a source change alter any kernel?  Compiles every csrc/*.hip of two source trees to device assembly (build.py's FLAGS plus
--cuda-device-only -S) and compares the two .s files line by line: kernel names, instruction streams and the .amdhsa_* register, LDS
and scratch values all have to match.  Only the lines that carry the __hip_cuid_<hash> symbol are dropped: that hash follows the file's
content and path, so it differs even between two compiles of one unchanged file from two directories.  Each tree's csrc/ and include/
are first copied to <work>/a and <work>/b, so both compile from the same directory depth.  A plain diff of compiler output; needs no GPU.

    python tests/tools/device_asm_diff.py <tree A> <tree B> [--flags "-DUNITER_X3_LAB ..."] [--keep <work dir>]

A tree is a checkout's root (e.g. `git worktree add /tmp/parent HEAD~1`).  Prints `equal` or the first differing lines per file, then the
compiler's warnings that are in one tree only; exits non-zero on any difference in the assembly."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', '..'))
from meme_challenge_amd.build import FLAGS, HIPCC


def stage(tree, dst):
    for sub in (os.path.join('meme_challenge_amd', 'csrc'), 'include'):
        shutil.copytree(os.path.join(tree, sub), os.path.join(dst, sub))
    return os.path.join(dst, 'meme_challenge_amd', 'csrc')


def device_asm(csrc, name, extra):
    out = os.path.join(csrc, name + '.s')
    r = subprocess.run([HIPCC] + FLAGS + extra + ['--cuda-device-only', '-S', name, '-o', out], cwd=csrc, capture_output=True, text=True)
    if r.returncode != 0:
        raise SystemExit('hipcc failed for %s:\n%s' % (os.path.join(csrc, name), r.stderr))
    with open(out) as f:
        return [l for l in f if '__hip_cuid_' not in l], [l for l in r.stderr.splitlines() if 'warning:' in l]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('tree_a')
    ap.add_argument('tree_b')
    ap.add_argument('--flags', default='', help='further compiler flags, e.g. a lab build\'s -D switches')
    ap.add_argument('--keep', help='work directory to keep the staged trees and .s files in')
    args = ap.parse_args()
    work = args.keep or tempfile.mkdtemp(prefix='device_asm_diff_')
    os.makedirs(work, exist_ok=True)
    try:
        csrc = [stage(t, os.path.join(work, d)) for t, d in ((args.tree_a, 'a'), (args.tree_b, 'b'))]
        names = [sorted(f for f in os.listdir(c) if f.endswith('.hip')) for c in csrc]
        jobs = [(c, n) for c, ns in zip(csrc, names) for n in ns]
        with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
            res = dict(zip(jobs, ex.map(lambda j: device_asm(j[0], j[1], args.flags.split()), jobs)))
    finally:
        if not args.keep:
            shutil.rmtree(work, ignore_errors=True)
    print('device assembly, A = %s, B = %s, flags: %s' % (args.tree_a, args.tree_b, ' '.join(FLAGS + args.flags.split())))
    differing = 0
    for n in sorted(set(names[0]) | set(names[1])):
        if n not in names[0] or n not in names[1]:
            differing += 1
            print('%-22s only in %s' % (n, 'A' if n in names[0] else 'B'))
            continue
        a, b = res[(csrc[0], n)][0], res[(csrc[1], n)][0]
        if a == b:
            print('%-22s equal (%d lines)' % (n, len(a)))
            continue
        differing += 1
        i = next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        print('%-22s DIFFERS from line %d (%d / %d lines)' % (n, i + 1, len(a), len(b)))
        for tag, ls in (('A', a), ('B', b)):
            for l in ls[i:i + 4]:
                sys.stdout.write('    %s: %s' % (tag, l))
    warn = [sorted(set(w for c_n, r in res.items() if c_n[0] == c for w in r[1])) for c in csrc]
    key = lambda w: re.sub(r':\d+:\d+:', ':', w)                # a moved line is not a new warning
    for tag, mine, other in (('A', warn[0], warn[1]), ('B', warn[1], warn[0])):
        for w in mine:
            if key(w) not in set(map(key, other)):
                print('warning only in %s: %s' % (tag, w))
    print('%d of %d files differ' % (differing, len(set(names[0]) | set(names[1]))))
    sys.exit(1 if differing else 0)


if __name__ == '__main__':
    main()
