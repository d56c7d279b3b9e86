"""Pool of oracle worker processes for the full-size GPU tests.

A spawned worker imports the module its function lives in.  This module imports nothing but numpy and the oracle, so
the workers never touch the GPU; a worker function kept in a `-m gpu` test module would open the device in every worker
through that module's `have_gpu()` marker, and a node allows only a few processes on its GPU at a time.
"""

import multiprocessing as mp
import os

import numpy as np


def _demod_worker(args):
    """The oracle's demodulator on one channel's IQ, two buffers."""
    kind, B, A, iqs = args
    import radiocore_oracle as oracle
    d = getattr(oracle, kind)(B, A)
    ch = 2 if kind == "WBFM" else 1
    return [np.asarray(d.run(iq)).reshape(A, ch).astype(np.float32) for iq in iqs]


def oracle_audio(kind, B, A, iq_per_channel):
    """{channel: [audio per buffer]} through a pool of oracle workers."""
    items = sorted(iq_per_channel.items())
    workers = max(1, min(32, (os.cpu_count() or 2) // 2, len(items)))
    ctx = mp.get_context("spawn")
    with ctx.Pool(workers) as pool:
        res = pool.map(_demod_worker, [(kind, B, A, iqs) for _, iqs in items], chunksize=1)
    return {c: r for (c, _), r in zip(items, res)}
