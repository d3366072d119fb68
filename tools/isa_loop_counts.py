#!/usr/bin/env python
"""Static instruction counts per kernel and per loop of one csrc/*.hip file, cross-compiled with the Makefile's flags (no GPU).

    python tools/isa_loop_counts.py wgrad_x6.hip [--kernel SUBSTRING] [--extra-flag=-fno-slp-vectorize ...] [--all-loops]
                                    [--makefile OTHER/Makefile] [--keep-asm out.s]

The file is compiled to gfx950 assembly with CXXFLAGS of sst_amd/csrc/Makefile plus the per-object `name.o: CXXFLAGS += ...`
lines of that file.  Every instruction is attributed to the innermost loop that LLVM's block comments name ("Loop Header",
"in Loop: Header=...") and classified BY PREFIX ONLY:
    mfma   v_mfma*              pk     v_pk_*  (packed arithmetic: the fp32 forms are the ones of interest beside MFMAs)
    valu   every other v_*      lds    ds_*    vmem   global_* buffer_* flat_* scratch_*      other  the rest (s_*, ...)
Loops without a matrix instruction are listed only with --all-loops.  Registers and scratch come from
-Rpass-analysis=kernel-resource-usage.  Counts are static: a loop body that holds several role branches counts all of them, and
they move with the compiler - a record, not a test."""
import argparse
import collections
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'sst_amd', 'csrc')
CLASSES = ('mfma', 'pk', 'valu', 'lds', 'vmem', 'other')


def makefile_flags(obj, makefile=None):
    """CXXFLAGS of the Makefile for object `obj` (name.o), $(ARCH) expanded"""
    text = open(makefile or os.path.join(CSRC, 'Makefile')).read()
    arch = re.search(r'^ARCH\s*\?=\s*(\S+)', text, re.M).group(1)
    flags = re.search(r'^CXXFLAGS\s*=\s*(.*)$', text, re.M).group(1).split()
    for m in re.finditer(r'^([^\n:#]+):\s*CXXFLAGS\s*\+=\s*(.*)$', text, re.M):
        if obj in m.group(1).split():
            flags += m.group(2).split()
    hipcc = os.environ.get('HIPCC') or re.search(r'^HIPCC\s*\?=\s*(\S+)', text, re.M).group(1)
    return hipcc, [f.replace('$(ARCH)', arch) for f in flags]


def classify(op):
    if op.startswith('v_mfma'):
        return 'mfma'
    if op.startswith('v_pk_'):
        return 'pk'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'buffer_', 'flat_', 'scratch_')):
        return 'vmem'
    return 'other'


def kernels(asm):
    """[(symbol, body lines)] of the functions of an AMDGPU assembly file"""
    out = []
    for m in re.finditer(r'^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:', asm, re.S | re.M):
        if '.amdhsa_kernel ' + m.group(1) in asm:
            out.append((m.group(1), m.group(2).split('\n')))
    return out


def loop_counts(lines):
    """{loop header label or None: Counter of classes} and {header: depth}; a block belongs to the loop its comments name"""
    counts = collections.defaultdict(collections.Counter)
    depth = {}
    cur = None
    pending = None          # label of a block whose comment lines are still being read
    for raw in lines:
        line = raw.strip()
        if not line:
            continue
        label = re.match(r'^(\.LBB\d+_\d+):', line) or re.match(r'^; %bb\.(\d+):', line)
        if label:
            pending = label.group(1).lstrip('.L') if line.startswith('.L') else None
            cur = None
        if label or line.startswith(';'):
            m = re.search(r'=>\s*This (?:Inner )?Loop Header: Depth=(\d+)', line)
            if m and pending:
                cur = pending
                depth[cur] = int(m.group(1))
            m = re.search(r'in Loop: Header=(BB\d+_\d+) Depth=(\d+)', line)
            if m:
                cur = m.group(1)
                depth[cur] = int(m.group(2))
            continue
        if line.startswith('.') or line.endswith(':'):
            continue
        counts[cur][classify(line.split()[0])] += 1
    return counts, depth


def resource_usage(stderr):
    """{mangled name: {'VGPRs': n, 'AGPRs': n, 'ScratchSize [bytes/lane]': n, ...}}"""
    out, name = {}, None
    for line in stderr.split('\n'):
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r'remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis', line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(['c++filt'] + names, capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.strip().split('\n')))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('source', help='a .hip file of sst_amd/csrc (name or path)')
    ap.add_argument('--kernel', default='', help='only kernels whose demangled name contains this')
    ap.add_argument('--extra-flag', action='append', default=[], help='appended to the Makefile flags (repeatable)')
    ap.add_argument('--all-loops', action='store_true', help='also list loops without a matrix instruction')
    ap.add_argument('--makefile', default=None, help='take the flags from this Makefile (e.g. the one of another revision)')
    ap.add_argument('--keep-asm', default=None, help='write the assembly to this file')
    a = ap.parse_args()
    src = a.source if os.path.exists(a.source) else os.path.join(CSRC, os.path.basename(a.source))
    obj = os.path.splitext(os.path.basename(src))[0] + '.o'
    hipcc, flags = makefile_flags(obj, a.makefile)
    flags += a.extra_flag
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, 'k.s')
        cmd = [hipcc] + flags + ['-I', CSRC, '--cuda-device-only', '-S', '-Rpass-analysis=kernel-resource-usage', src, '-o', out]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit('compile failed: %s\n%s' % (' '.join(cmd), r.stderr[-4000:]))
        asm = open(out).read()
    if a.keep_asm:
        open(a.keep_asm, 'w').write(asm)
    usage = resource_usage(r.stderr)
    ks = kernels(asm)
    names = demangle([k for k, _ in ks])
    print('# %s   flags: %s' % (os.path.basename(src), ' '.join(flags)))
    for sym, lines in ks:
        name = names[sym]
        if a.kernel not in name:
            continue
        counts, depth = loop_counts(lines)
        total = collections.Counter()
        for c in counts.values():
            total.update(c)
        u = usage.get(sym, {})
        print('\n%s' % name)
        print('  VGPRs %s  AGPRs %s  SGPRs %s  scratch %s B/lane  occupancy %s waves/SIMD' % (
            u.get('VGPRs', '?'), u.get('AGPRs', '?'), u.get('TotalSGPRs', '?'), u.get('ScratchSize [bytes/lane]', '?'),
            u.get('Occupancy [waves/SIMD]', '?')))
        print('  %-22s' % 'where' + ''.join('%8s' % c for c in CLASSES))
        print('  %-22s' % 'whole kernel' + ''.join('%8d' % total[c] for c in CLASSES))
        for hdr in sorted((h for h in counts if h), key=lambda h: int(h.split('_')[1])):
            c = counts[hdr]
            if c['mfma'] or a.all_loops:
                print('  %-22s' % ('loop %s depth %d' % (hdr, depth.get(hdr, 0))) + ''.join('%8d' % c[k] for k in CLASSES))
        mf = [h for h in counts if h and counts[h]['mfma']]
        bad = [h for h in mf if counts[h]['pk']]
        print('  loops with MFMA: %d, of them with packed (v_pk_*) instructions: %d' % (len(mf), len(bad)))


if __name__ == '__main__':
    main()
