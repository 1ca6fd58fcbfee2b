"""Builds libapgpu.so (the HIP kernels + C ABI, include/apgpu.h) for gfx950 with hipcc.

``python -m astrophotography_amd._build`` or ``__graft_entry__.build()``.  hipcc cross-compiles without
a GPU; the .so is written next to this file so that it travels with the source tree.
"""
import concurrent.futures as cf
import os
import re
import shlex
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, 'csrc')
OBJ = os.path.join(CSRC, '_obj')
LIB = os.path.join(PKG, 'libapgpu.so')

# The translation units, in link order.  First the ones that are a source file each ...
UNITS = ['common', 'elementwise', 'fixbadpix', 'sigclip_global', 'resample', 'resample_stack', 'stack', 'stack_big', 'stack_chunks',
         'stack_mad', 'stack_mad_wide', 'stack_mad_pairs', 'stack_mad_pairs_wide', 'combine_f64', 'background', 'lacosmic', 'autobadcol', 'findstars',
         'measurestars', 'register', 'composite', 'demosaic', 'continuum', 'deconvolve', 'multiscale', 'drizzle']
# ... then the register-resident stack kernels: stack_inst.hip once per slot group x raw dtype x fused calibration (the groups'
# slot counts: the table in stack_calibrate.h).  The groups are linked in the fatbinary order of the library the recorded
# measurements were taken with (largest slot counts first): a kernel's place in the loaded code is kept with it.
STACK_GROUPS = ['h', 'o', 'g', 'j', 'f', 'n', 'e', 'i', 'd', 'm', 'c', 'l', 'b', 'k', 'a']
STACK_DTYPES = [('f32', 'float'), ('u16', 'uint16_t')]
STACK_CALIB = [('calib', 'true'), ('plain', 'false')]
# ... and, behind them (so that every older kernel keeps its place in the loaded code), the units added since.
LATE_UNITS = ['stack_reject']
# ... the last of them once per raw dtype: the ESD rule's kernels (stack_esd.hip)
ESD_UNITS = [('stack_esd_' + tag, 'stack_esd', ['-DAPGPU_ESD_RAW=' + raw, '-DAPGPU_ESD_ENTRY=launch_esd_' + tag]) for tag, raw in STACK_DTYPES]
# ... and the lens distortion's own unit (its other kernels are instances of the register and drizzle units' templates)
DISTORTION_UNITS = [('distortion', 'distortion', [])]
# ... and the sky gradient's unit (its sample statistics are an instance of box_stats.h's kernel, which background.hip shares)
GRADIENT_UNITS = [('gradient', 'gradient', [])]
# ... and the plate solver's catalogue kernels (its votes and neighbour searches are the register unit's)
ASTROMETRY_UNITS = [('astrometry', 'astrometry', [])]
# ... and the empirical PSF's unit (its interpolant: epsf_core.h)
EPSF_UNITS = [('epsf', 'epsf', [])]
# ... and the optimal image subtraction's unit (its basis and spatial polynomials: subtract_core.h)
SUBTRACT_UNITS = [('subtract', 'subtract', [])]

# -ffp-contract=off: the reference's NumPy expressions round after every operation, so no FMA
# contraction anywhere; fused operations are written explicitly (fma()) where wanted.
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-ffp-contract=off', '-fno-fast-math', '-Wall',
               '-Wno-unused-function', '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC]
# The stack kernels' translation units: machine LICM off - the complete lean kernel is one loop (plain launch and redo pass share
# its body) and hoisted loop-invariant values cost it 5-10 VGPRs, the difference between three and two wavefronts per SIMD.
STACK_TU_FLAGS = ['-mllvm', '-disable-machine-licm']


def _hipcc():
    for cand in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', 'hipcc'):
        if cand and (os.path.isabs(cand) and os.path.exists(cand) or not os.path.isabs(cand)):
            return cand
    return 'hipcc'


def compile_units(obj_dir=OBJ):
    """Yields (unit name, source, full compile command) in link order; the object is <obj_dir>/<unit name>.o, and the compiler
    writes the files it read next to it (<unit name>.d)."""
    base = [_hipcc()] + (['-DAPGPU_DEVELOPMENT'] if os.environ.get('APGPU_DEVELOPMENT') else []) + HIPCC_FLAGS
    units = [(u, u, STACK_TU_FLAGS if u == 'resample_stack' else []) for u in UNITS]
    units += [('stack_inst_%s_%s_%s' % (tag, ctag, g), 'stack_inst',
               STACK_TU_FLAGS + ['-DAPGPU_INST_RAW=' + raw, '-DAPGPU_INST_CALIB=' + calib, '-DAPGPU_INST_GROUP=' + g])
              for g in STACK_GROUPS for tag, raw in STACK_DTYPES for ctag, calib in STACK_CALIB]
    units += [(u, u, []) for u in LATE_UNITS] + ESD_UNITS + DISTORTION_UNITS + GRADIENT_UNITS + ASTROMETRY_UNITS + EPSF_UNITS + SUBTRACT_UNITS
    for name, src, flags in units:
        stem = os.path.join(obj_dir, name)
        srcp = os.path.join(CSRC, src + '.hip')
        yield name, srcp, base + flags + ['-MD', '-MF', stem + '.d', '-c', srcp, '-o', stem + '.o']


def _up_to_date(obj, cmdline):
    """The object is newer than every file the compiler read for it, and was made by this very command line."""
    try:
        if open(obj[:-2] + '.cmd').read() != cmdline:
            return False
        deps = open(obj[:-2] + '.d').read().replace('\\\n', ' ').split(': ', 1)[1]
        built = os.path.getmtime(obj)
        return all(os.path.getmtime(d.replace('\\ ', ' ')) <= built for d in re.split(r'(?<!\\)\s+', deps.strip()))
    except (OSError, IndexError):                            # no object, stamp or dependency file, or a file it names is gone
        return False


def _compile(unit):
    name, _, cmd = unit
    obj, cmdline = cmd[-1], shlex.join(cmd)
    if _up_to_date(obj, cmdline):
        return obj, False
    stamp = obj[:-2] + '.cmd'
    if os.path.exists(stamp):
        os.remove(stamp)                                     # (an interrupted compile leaves no stamp: built again)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed for %s:\n%s' % (name, r.stdout[-4000:]))
    with open(stamp, 'w') as fh:
        fh.write(cmdline)
    return obj, True


def build_library(force=False, verbose=False, jobs=None):
    os.makedirs(OBJ, exist_ok=True)
    if force:
        for f in os.listdir(OBJ):
            os.remove(os.path.join(OBJ, f))
    units = list(compile_units())
    jobs = jobs or int(os.environ.get('MAX_JOBS') or 0) or min(len(units), os.cpu_count() or 4, 16)
    with cf.ThreadPoolExecutor(jobs) as ex:
        results = list(ex.map(_compile, units))
    objs = [o for o, _ in results]
    rebuilt = any(r for _, r in results)
    if rebuilt or not os.path.exists(LIB) or os.path.getmtime(LIB) < max(map(os.path.getmtime, objs)):
        cmd = [_hipcc(), '--offload-arch=gfx950', '-shared', '-fPIC', '-o', LIB] + objs
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError('link failed:\n%s' % r.stdout[-4000:])
    if verbose:
        print('libapgpu.so %s' % ('rebuilt' if rebuilt else 'up to date'), LIB)
    return LIB


if __name__ == '__main__':
    if '--commands' in sys.argv:                             # one line per unit: name, source, command (for tools/*.sh)
        obj_dir = sys.argv[sys.argv.index('--obj-dir') + 1] if '--obj-dir' in sys.argv else OBJ
        for name, src, cmd in compile_units(obj_dir):
            print('%s\t%s\t%s' % (name, src, shlex.join(cmd)))
    else:
        build_library(force='--force' in sys.argv, verbose=True)
