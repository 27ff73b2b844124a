"""Posterior summaries of saved runs on the GPU (the numerical half of the reference's
musefuse_postprocess.py:112-140 and checkoutput.py:27-44; the plotting stays out).

    python -m massivedatans_amd.postprocess OUT [OUT ...] [--quantiles 0.16,0.5,0.84]
                                            [--resample N --seed S] [-o PATH] [--quiet]

``OUT``: a file ``save_results`` wrote (``<prefix>.npz``, or ``<prefix>.hdf5`` where h5py is installed).
The ``<prefix>.cols<lo>-<hi>.*`` parts of a sharded run are summarised part by part and written as ONE
file in column order; parts that leave a gap or overlap are refused.  Writes ``<prefix>.posterior.npz``:
``nfinite``, ``log_norm``, ``ess``, ``mean``, ``std``, ``quant``, ``imaxL``, ``q``, ``logZ``, ``logZerr``,
``columns`` and, with ``--resample``, ``index`` (rows of the run, ``[ndata, N]``) and ``seed``.
"""
import argparse
import os
import re
import sys

import numpy as np

_PART = re.compile(r'^(?P<prefix>.*)\.cols(?P<lo>\d+)-(?P<hi>\d+)$')
_SUFFIXES = ('.npz', '.hdf5', '.h5')


def _split(path):
    """(prefix, lo, hi) of an output file; lo = hi = None for a file that is not a .cols part."""
    stem = path
    for s in _SUFFIXES:
        if stem.endswith(s):
            stem = stem[:-len(s)]
            break
    m = _PART.match(stem)
    if m is None:
        return stem, None, None
    return m.group('prefix'), int(m.group('lo')), int(m.group('hi'))


def plan_parts(paths):
    """Group output files into summaries: ``[(prefix, [(path, lo, hi), ...]), ...]``.  A whole file is a
    group of its own (lo = hi = None); the ``.cols<lo>-<hi>`` parts of one prefix form one group in column
    order.  Raises ``ValueError`` when parts of a prefix overlap or leave a gap, or a prefix is given both
    whole and in parts."""
    groups, order = {}, []
    for p in paths:
        prefix, lo, hi = _split(p)
        if lo is not None and hi <= lo:
            raise ValueError("%s: empty column range %d-%d" % (p, lo, hi))
        key = (prefix, lo is None)
        if key not in groups:
            groups[key] = []
            order.append(key)
        groups[key].append((p, lo, hi))
    out = []
    for prefix, whole in order:
        members = groups[(prefix, whole)]
        if whole:
            if (prefix, False) in groups:
                raise ValueError("%s is given both whole and in .cols parts" % prefix)
            for m in members:
                out.append((prefix, [m]))
            continue
        members = sorted(members, key=lambda m: (m[1], m[2]))
        for a, b in zip(members, members[1:]):
            if b[1] < a[2]:
                raise ValueError("parts overlap: %s (columns %d-%d) and %s (columns %d-%d)" % (a[0], a[1], a[2], b[0], b[1], b[2]))
            if b[1] > a[2]:
                raise ValueError("gap between parts: columns %d-%d are missing (%s, %s)" % (a[2], b[1], a[0], b[0]))
        out.append((prefix, members))
    return out


def summarize_file(path, quantiles, resample=0, seed=1, first_column=0):
    """The posterior summary of one output file (see ``posterior.summarize_results``)."""
    from . import gen
    from .posterior import Posterior
    data = gen.read_datasets(path)
    with Posterior(data['w'], data['L'], data['x']) as post:
        out = post.summary(quantiles)
        if resample:
            out['index'] = post.resample(resample, seed=seed, first_column=first_column)
            out['seed'] = np.uint64(seed)
    out['logZ'] = np.atleast_1d(data['logZ'])
    out['logZerr'] = np.atleast_1d(data['logZerr'])
    return out


def merge(parts):
    """Per-data-set arrays of several column ranges, in the order given, as one summary."""
    first = parts[0]
    out = {}
    for k, v in first.items():
        if k in ('q', 'seed'):
            out[k] = v
        else:
            out[k] = np.concatenate([p[k] for p in parts], axis=0)
    return out


def summarize_group(members, quantiles, resample=0, seed=1):
    parts = [summarize_file(path, quantiles, resample, seed, first_column=lo or 0) for path, lo, hi in members]
    out = merge(parts)
    lo = members[0][1] or 0
    out['columns'] = np.array([lo, lo + len(out['nfinite'])])
    return out


def write(path, out):
    np.savez(path, **out)


def report(out, names=None, stream=sys.stdout):
    """A few lines per data set, as the reference's loop prints them."""
    nd, ndim = out['mean'].shape
    lo = int(out['columns'][0])
    for d in range(nd):
        print('   %d/%d: data set %d: %d finite samples, effective %.1f' % (d + 1, nd, lo + d, out['nfinite'][d], out['ess'][d]),
              file=stream)
        print('        logZ = %.1f +- %.1f' % (out['logZ'][d], out['logZerr'][d]), file=stream)
        for k in range(ndim):
            qs = ' '.join('%.3f' % v for v in out['quant'][d, k])
            print('          param %d = %.3f +- %.3f  quantiles %s' % (k, out['mean'][d, k], out['std'][d, k], qs), file=stream)


def run_posterior_outputs(prefix, results):
    """``MDNS_POSTERIOR=N`` (unset: nothing): the posterior file of a finished run next to its outputs,
    N > 0 draws per data set with seed 1 (0: summaries only).  A sharded rank (``columns`` in the
    results) writes ``<prefix>.cols<lo>-<hi>.posterior.npz`` of its own data sets on its own GPU; an
    unsharded run writes ``<prefix>.posterior.npz`` on rank 0."""
    n = os.environ.get('MDNS_POSTERIOR')
    if n is None or n == '':
        return None
    from .posterior import summarize_results
    if 'columns' in results:
        lo, hi = results['columns']
        path = '%s.cols%d-%d.posterior.npz' % (prefix, lo, hi)
    elif int(os.environ.get('RANK', '0')) == 0:
        path = prefix + '.posterior.npz'
    else:
        return None
    write(path, summarize_results(results, resample=int(n), seed=1))
    return path


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m massivedatans_amd.postprocess', description=__doc__.split('\n')[0])
    ap.add_argument('outputs', nargs='+', help='files save_results wrote (.npz / .hdf5), or the .cols parts of a sharded run')
    ap.add_argument('--quantiles', default='0.16,0.5,0.84', help='comma-separated probabilities in (0, 1]')
    ap.add_argument('--resample', type=int, default=0, metavar='N', help='equal-weight draws per data set')
    ap.add_argument('--seed', type=int, default=1)
    ap.add_argument('-o', '--output', default=None, help='output path (one group of inputs only)')
    ap.add_argument('--quiet', action='store_true', help='no per-data-set lines')
    args = ap.parse_args(argv)
    from ._lib import MdnsError
    quantiles = [float(v) for v in args.quantiles.split(',') if v.strip()]
    try:
        groups = plan_parts(args.outputs)
    except ValueError as e:
        sys.exit('postprocess: %s' % e)
    if args.output and len(groups) != 1:
        sys.exit('postprocess: -o needs the inputs to form one summary (got %d)' % len(groups))
    for prefix, members in groups:
        try:
            out = summarize_group(members, quantiles, args.resample, args.seed)
        except MdnsError as e:
            sys.exit('postprocess: %s' % e)
        path = args.output or prefix + '.posterior.npz'
        write(path, out)
        if not args.quiet:
            report(out)
        print('%s: %d data sets from %d file(s) -> %s' % (prefix, len(out['nfinite']), len(members), path))


if __name__ == '__main__':
    main()
