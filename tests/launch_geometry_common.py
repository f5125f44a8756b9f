"""The launch-geometry settings tests/test_gpu_launch_geometry.py sweeps, and the host arithmetic they force into play -- in a module of
their own so that tests/test_tuning_ranges_host.py can check, without a GPU, that fn_set_tuning accepts every one of them.

Every attention kernel gives a half-wave ``rows_per_hw`` consecutive rows of its level and a block eight half-waves:

    rows_per_hw = ceil(ceil(n / 8) / blocks)          nblk = ceil(n / (8 * rows_per_hw))

with ``blocks`` the value of the pass's tuning key (include/fragnet_hip.h FN_TUNE_*).  At the defaults (sized for 512 molecules) a batch
of 4 - 96 molecules has fewer row groups than blocks at every level: rows_per_hw == 1 everywhere."""

ROWS = 8                                   # rows of a block of the attention kernels (kRows, kBwdRows)
EDGES_ROWS = dict(bond=1330, atom=712, fbond=549, frag=314)      # the "edges" batch of tests/topologies.py (asserted from its plan)

FWD_BLOCKS, GEMM_SLOTS, WGRAD_BLOCKS, FWD_BLOCKS_EVAL, DST_BLOCKS, SRC_BLOCKS, RD_BLOCKS = 0, 1, 3, 10, 11, 12, 13
WGRAD0_ROWS, BWD_ONE, ONE_BLOCKS, PAD_SKIP, ONE_INTERLEAVE = 21, 22, 23, 24, 25


def geometry(n, blocks):
    """(rows_per_hw, nblk) of a level of ``n`` rows under a block target of ``blocks``."""
    groups = -(-n // ROWS)
    rows_per_hw = -(-groups // blocks)
    return rows_per_hw, -(-n // (ROWS * rows_per_hw))


ONE_BLOCKS_VALUES = (1, 2, 7, 40, 56, 166, 167)

# a. one training step without dropout, gradients against the oracle
BACKWARD_SETTINGS = (
    [{ONE_BLOCKS: v} for v in ONE_BLOCKS_VALUES]
    + [{ONE_INTERLEAVE: 1}, {ONE_INTERLEAVE: 1, ONE_BLOCKS: 7}]
    + [{BWD_ONE: 0, SRC_BLOCKS: v} for v in (1, 3, 40, 1024)]
    + [{BWD_ONE: 0, DST_BLOCKS: v} for v in (1, 40, 4095)]
    + [{RD_BLOCKS: v} for v in (1, 3, 4096)]
    + [{WGRAD_BLOCKS: v} for v in (1, 2, 4096)]
    + [{WGRAD0_ROWS: v} for v in (11, 13, 31, 99)]
    + [{GEMM_SLOTS: v} for v in (2, 8, 1024)])

# b. the training forward (dropout epilogue)
FWD_BLOCKS_VALUES = (1, 2, 5, 23)

# c. the operators
LINEAR_SLOTS = (1, 2, 3, 1024)
LEVEL_BLOCKS = (1, 2, 4, 9)                # a level of 70 rows has 9 row groups
LEVEL_SETTINGS = {True: [{FWD_BLOCKS_EVAL: v, ONE_BLOCKS: v} for v in LEVEL_BLOCKS],        # ops.BWD_ONE_PASS -> the keys of its passes
                  False: [{DST_BLOCKS: v, SRC_BLOCKS: v} for v in LEVEL_BLOCKS]}

# d. the captured step on a padded batch
PAD_SKIP_VALUES = (1, 0)


def all_settings():
    """Every {key: value} a GPU test of the sweep sets."""
    out = list(BACKWARD_SETTINGS) + [{FWD_BLOCKS: v} for v in FWD_BLOCKS_VALUES] + [{GEMM_SLOTS: v} for v in LINEAR_SLOTS]
    out += LEVEL_SETTINGS[True] + LEVEL_SETTINGS[False] + [{PAD_SKIP: v} for v in PAD_SKIP_VALUES]
    return out


def sid(setting):
    return "_".join(f"{k}={v}" for k, v in setting.items())
