"""The accepting-state rule of lstm_hip_generate_accepting (include/lstm_hip.h) in numpy, on
tests/constraint_ref.py and tests/beam_constraint_ref.py: a byte EXISTS at a draw with R draws left iff the table allows it and
it leads where an accepted end can still be reached (F[R - 1] of beam_constraint_ref.f_table), or, for the stop byte, into an
accepting state.  A draw is constraint_ref's draw on the row that forbids what does not exist."""
import numpy as np

import beam_constraint_ref as bc
import constraint_ref as cr

FORBID = cr.FORBID
f32 = np.float32


def exists(table, accept, F, stop, q, R):
    """[256] bool: the bytes that exist in state q with R draws left (R >= 1)"""
    row = np.asarray(table[q]).astype(np.int64)
    ok = row != FORBID
    nx = np.where(ok, row, 0)
    ex = ok & np.asarray(F[R - 1])[nx]
    if stop >= 0:
        ex[stop] = ok[stop] and bool(accept[nx[stop]])
    return ex


def row_of(table, accept, F, stop, q, R):
    """a one-state table: state q's row with every byte that does not exist forbidden"""
    return np.where(exists(table, accept, F, stop, q, R), np.asarray(table[q]), FORBID).astype(np.uint16)[None, :]


def draw32(z, table, accept, F, stop, q, R, mode, tau, top_k, top_p, u):
    """one draw as the head computes it from the float32 logits z: (byte, kept)"""
    return cr.draw32(z, row_of(table, accept, F, stop, q, R), 0, mode, tau, top_k, top_p, u)


def filter64(p1, table, accept, F, stop, q, R, tau, top_k, top_p):
    """constraint_ref.filter64 over the bytes that exist"""
    return cr.filter64(p1, row_of(table, accept, F, stop, q, R), 0, tau, top_k, top_p)


def ambiguous(p, table, accept, F, stop, q, R, top_k, top_p):
    return cr.ambiguous(p, row_of(table, accept, F, stop, q, R), 0, top_k, top_p)


def pack_rows(F):
    """the rows as the head reads them: [R][words] uint32, bit q % 32 of word q / 32"""
    F = np.asarray(F, bool)
    words = (F.shape[1] + 31) // 32
    out = np.zeros((F.shape[0], words), np.uint32)
    for q in range(F.shape[1]):
        out[:, q >> 5] |= F[:, q].astype(np.uint32) << np.uint32(q & 31)
    return out


def f_table(table, accept, stop, count):
    return bc.f_table(table, accept, stop, count)


# ---- the case of the GPU oracle comparison (tests/test_generate_accepting.py) and of its CPU control
# (tests/test_accepting_cpu.py): constraint_ref's eight-stream case under the UTF-8 table with the character boundary as
# the only accepting state, and sampling_ref's four ASCII-prompted streams under printable ASCII with a newline as stop byte
ORACLE_TABLES = ("utf8_accept", "ascii_stop")
ORACLE_COUNT = 60


def oracle_case(name, utf8_table):
    """(P, prompts, u [ORACLE_COUNT, streams], table, accept, stop byte)"""
    import sampling_ref as sr
    table, accept, stop = bc.oracle_table(name, utf8_table)
    if accept is None:
        accept = np.ones(table.shape[0], np.uint8)
    if name == "utf8_accept":
        P, prompts, u = cr.oracle_case()
    else:
        P, prompts, u = sr.oracle_case()
    return P, prompts, u[:ORACLE_COUNT], table, accept, stop
