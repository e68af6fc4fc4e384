"""Shared cases of the mini-batch trainer's tests.  A case is (name, kwargs) for
train(rows, labels, unlabelled, n1, n2, minmax, init, batch, **opts); unlabelled None: the supervised trainer (train_mlp_batches).  Host
cases are compared with the second author tests/_batchdef.py (reference(), computed once per case); GPU cases compare the device with
the host trainer."""
import numpy as np

import _batchdef as B
import _mlptrain_cases as MK
import _sshmt_cases as K

DIM = 5
ROWS, LABELS = MK._data(150, DIM, 4)          # 150 labelled rows: batches of 70 are a 64-row and a 6-row chunk; three draws an epoch
# two unlabelled blocks of 40 merges: 38 + 38 paths of 3 members at (3, 2); row r lies on paths r, r - 1, r - 2 of its block
BLOCKS = [K._block(K.caterpillar(40), DIM, 1), K._block(K.caterpillar(40, key0=500), DIM, 2)]
LOGSIG_INIT = np.linspace(-0.3, 0.3, DIM + 1)
LOGSIG_INIT.setflags(write=False)
BASE = dict(MK.BASE, sup_batch_size=70)       # wr 0.01, ws 1, sigma_s 0.5, step 0.05, 3 iterations, 2 rounds
UBASE = dict(BASE, wu=0.5, sigma_u=0.7)


def _case(name, unlabelled, n1, n2, batch=None, rows=ROWS, labels=LABELS, init=None, **opts):
    return name, dict(rows=rows, labels=labels, unlabelled=unlabelled, n1=n1, n2=n2, minmax=None, init=init, batch=dict(batch or {}), opts=opts)


def host_cases():
    out = []
    for opt in (1, 2, 3):
        out.append(_case("mlp_fixed_opt%d" % opt, None, 3, 3, dict(seed=opt), **dict(BASE, optimizer=opt, seed=opt)))
        out.append(_case("logsig_adaptive_opt%d" % opt, None, 0, 0, dict(seed=10 + opt), init=LOGSIG_INIT, **dict(BASE, optimizer=opt, step_decay=0.5)))
    # a step so large that the first try cannot lower the energy: the roll-back draws new batches
    out.append(_case("mlp_rollback", None, 3, 3, dict(seed=5), **dict(BASE, optimizer=1, step=1e3, step_decay=0.25, seed=2)))
    out.append(_case("mlp_te2", None, 3, 3, dict(seed=6, epochs_per_iteration=2), **dict(BASE, optimizer=2)))
    out.append(_case("logsig_tb3", None, 0, 0, dict(seed=7, epochs_per_iteration=0, batches_per_iteration=3), init=LOGSIG_INIT, **dict(BASE, optimizer=3)))
    out.append(_case("mlp_balanced", None, 3, 3, dict(seed=8), **dict(BASE, balance_sup_batch=1, sup_batch_size=41)))
    out.append(_case("mlp_balanced_all_minority", None, 3, 3, dict(seed=9), **dict(BASE, balance_sup_batch=1, sup_batch_size=-1, pos_target=0.9, neg_target=0.1)))
    # the path term: its sampler alone, the row sampler alone, both (76 paths: two draws end the epoch before the rows' three)
    out.append(_case("paths_only_sampler", BLOCKS, 3, 3, dict(seed=11), **dict(UBASE, sup_batch_size=-1, uns_batch_size=70, optimizer=2)))
    out.append(_case("rows_only_sampler", BLOCKS, 3, 3, dict(seed=12), **dict(UBASE, optimizer=3)))
    out.append(_case("both_samplers", BLOCKS, 3, 3, dict(seed=13), **dict(UBASE, uns_batch_size=70, optimizer=1, step_decay=0.5)))
    out.append(_case("both_samplers_logsig_tb3", BLOCKS, 0, 0, dict(seed=14, epochs_per_iteration=0, batches_per_iteration=3), init=LOGSIG_INIT,
                     **dict(UBASE, uns_batch_size=70, optimizer=2)))
    out.append(_case("paths_only_no_labelled", BLOCKS, 3, 3, dict(seed=15), rows=None, labels=None,
                     **dict(UBASE, ws=0.0, wr=0.0, sup_batch_size=-1, uns_batch_size=70)))
    return out


HOST = host_cases()
HOST_IDS = [n for n, _ in HOST]
_REF = {}


def host_kw(name):
    return HOST[HOST_IDS.index(name)][1]


def reference(name):
    if name not in _REF:
        kw = host_kw(name)
        _REF[name] = B.train(kw["rows"], kw["labels"], kw["unlabelled"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], kw["batch"], **kw["opts"])
    return _REF[name]


def train(hmt, ctx, kw, **more):
    """the library's trainer for a case: train_mlp_batches without unlabelled blocks, train_sshmt_batches with"""
    o = dict(kw["opts"])
    o.update(more)
    if kw["unlabelled"] is None:
        return hmt.train_mlp_batches(ctx, kw["rows"], kw["labels"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], kw["batch"], **o)
    return hmt.train_sshmt_batches(ctx, kw["rows"], kw["labels"], kw["unlabelled"], kw["n1"], kw["n2"], kw["minmax"], kw["init"], kw["batch"], **o)


def gpu_cases():
    """the smallest shapes that reach every branch of the device path"""
    out = []
    i = 0
    for bss in (1, 64, 65):                                   # one row; a whole chunk; a chunk and a row
        for n1, n2 in ((16, 16), (17, 17)):                   # both NMAX instances of the chunk kernel
            out.append(_case("sup_b%d_%d_%d" % (bss, n1, n2), None, n1, n2, dict(seed=i, epochs_per_iteration=0, batches_per_iteration=3),
                             **dict(BASE, sup_batch_size=bss, optimizer=1 + i % 3, seed=i)))
            i += 1
    out.append(_case("sup_logsig_epoch", None, 0, 0, dict(seed=20), init=LOGSIG_INIT, **dict(BASE, optimizer=2)))
    out.append(_case("sup_balanced", None, 3, 3, dict(seed=21), **dict(BASE, balance_sup_batch=1, sup_batch_size=41, optimizer=3)))
    for bsu in (64, 65):                                      # path chunks; 65 caterpillar paths name more than 64 rows
        out.append(_case("paths_b%d" % bsu, BLOCKS, 3, 17, dict(seed=22 + bsu), **dict(UBASE, sup_batch_size=-1, uns_batch_size=bsu, optimizer=2)))
    out.append(_case("both_samplers", BLOCKS, 16, 16, dict(seed=30), **dict(UBASE, uns_batch_size=70, optimizer=3)))
    out.append(_case("rows_only_sampler", BLOCKS, 3, 3, dict(seed=31), **dict(UBASE, optimizer=1)))
    out.append(_case("paths_logsig", BLOCKS, 0, 0, dict(seed=32, epochs_per_iteration=2), init=LOGSIG_INIT,
                     **dict(UBASE, sup_batch_size=-1, uns_batch_size=64, optimizer=1)))
    out.append(_case("rollback", BLOCKS, 3, 3, dict(seed=5), **dict(UBASE, uns_batch_size=70, optimizer=1, step=1e3, step_decay=0.25, seed=2)))
    return out


GPU = gpu_cases()
GPU_IDS = [n for n, _ in GPU]
