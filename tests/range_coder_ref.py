"""A pure-Python copy of the device's range coder (eigen-lstm_amd/csrc/heads/code_head.inc, rc_* and k_code_head; DESIGN.md
section 3.6): the carryless 32-bit coder (Subbotin), TOP = 2^24, BOT = 2^16, a 4-byte flush, totals <= 2^16, at most three
byte moves per coded symbol.  Test helper: it re-encodes a device trace of (cum, freq, total) and decodes codes back.
encode and decode take an optional Stats, which counts the paths a run took and keeps the coder's final state; it changes
no result."""
TOP = 1 << 24
BOT = 1 << 16
MASK = 0xFFFFFFFF
MAX_SHIFTS = 3


class CoderError(RuntimeError):
    """the device would flag this call (a total above 2^16, or a fourth byte move in one step)"""


class Stats:
    """cuts: steps that took the carryless cut; moves: the byte moves of every step, max_moves the most of them; clamps:
    decode steps whose (code - low) / r was >= T and was clamped to T - 1; and the state after the last step as the device
    keeps it: low, range, code (decoder), pos (code bytes written or read, the encoder's four flush bytes included)."""

    def __init__(self):
        self.cuts = self.max_moves = self.clamps = 0
        self.moves = []
        self.low = self.range = self.code = self.pos = None


def _normalize(low, rng, move, stats=None):
    n = 0
    cut = False
    while True:
        if (low ^ ((low + rng) & MASK)) >= TOP:  # top bytes differ
            if rng >= BOT:
                if stats is not None:
                    stats.moves.append(n)
                    stats.cuts += cut
                    stats.max_moves = max(stats.max_moves, n)
                return low, rng
            rng = (-low) & (BOT - 1)  # the carryless cut
            cut = True
        if n == MAX_SHIFTS:
            raise CoderError("more than three byte moves in one step")
        move(low >> 24)
        low = (low << 8) & MASK
        rng = (rng << 8) & MASK
        n += 1


def encode(symbols, stats=None):
    """symbols: iterable of (cum, freq, total).  Returns the code (empty for no symbols)."""
    out = bytearray()
    low, rng, n = 0, MASK, 0
    for cum, freq, total in symbols:
        cum, freq, total = int(cum), int(freq), int(total)
        if total > BOT or freq < 1 or cum + freq > total:
            raise CoderError(f"bad symbol ({cum}, {freq}, {total})")
        r = rng // total
        low = (low + cum * r) & MASK
        rng = (freq * r) & MASK
        low, rng = _normalize(low, rng, out.append, stats)
        n += 1
    if n:
        for _ in range(4):
            out.append(low >> 24)
            low = (low << 8) & MASK
    if stats is not None and n:
        stats.low, stats.range, stats.code, stats.pos = low, rng, 0, len(out)
    return bytes(out)


def decode(code, count, model, stats=None):
    """Decodes `count` symbols.  model(i) -> (total, find) for step i, where find(v) gives (symbol, cum, freq) of the
    interval holding v (cum <= v < cum + freq).  Bytes past the end of `code` read as 0.  Returns the symbols."""
    pos = 0

    def get():
        nonlocal pos
        b = code[pos] if pos < len(code) else 0
        pos += 1
        return b

    low, rng, c = 0, MASK, 0
    out = []
    for i in range(count):
        if i == 0:
            for _ in range(4):
                c = ((c << 8) | get()) & MASK
        total, find = model(i)
        if total > BOT:
            raise CoderError(f"total {total} above 2^16")
        rng //= total
        v = ((c - low) & MASK) // rng
        if v >= total:
            v = total - 1
            if stats is not None:
                stats.clamps += 1
        sym, cum, freq = find(v)
        low = (low + cum * rng) & MASK
        rng = (freq * rng) & MASK

        def move(_byte):
            nonlocal c
            c = ((c << 8) | get()) & MASK

        low, rng = _normalize(low, rng, move, stats)
        out.append(sym)
    if stats is not None and count:
        stats.low, stats.range, stats.code, stats.pos = low, rng, c, pos
    return out


def table_model(tables):
    """model for decode() from full frequency tables: tables[i] is the list of q_m of step i (cum by prefix sum)."""
    import bisect
    import itertools

    cums = [list(itertools.accumulate(q, initial=0)) for q in tables]

    def model(i):
        cum = cums[i]

        def find(v):
            m = bisect.bisect_right(cum, v) - 1
            return m, cum[m], cum[m + 1] - cum[m]

        return cum[-1], find

    return model


def trace_model(trace, symbols):
    """model for decode() from a device trace: step i must land in the traced interval, whose symbol is symbols[i]."""
    def model(i):
        cum, freq, total = (int(x) for x in trace[i])

        def find(v):
            if not cum <= v < cum + freq:
                raise CoderError(f"step {i}: value {v} outside the traced interval [{cum}, {cum + freq})")
            return int(symbols[i]), cum, freq

        return total, find

    return model
