"""A pure-Python copy of the device's range coder (eigen-lstm_amd/csrc/heads/code_head.inc, rc_* and k_code_head; DESIGN.md
section 3.6): the carryless 32-bit coder (Subbotin), TOP = 2^24, BOT = 2^16, a 4-byte flush, totals <= 2^16, at most three
byte moves per coded symbol.  Test helper: it re-encodes a device trace of (cum, freq, total) and decodes codes back."""
TOP = 1 << 24
BOT = 1 << 16
MASK = 0xFFFFFFFF
MAX_SHIFTS = 3


class CoderError(RuntimeError):
    """the device would flag this call (a total above 2^16, or a fourth byte move in one step)"""


def _normalize(low, rng, move):
    n = 0
    while True:
        if (low ^ ((low + rng) & MASK)) >= TOP:  # top bytes differ
            if rng >= BOT:
                return low, rng
            rng = (-low) & (BOT - 1)  # the carryless cut
        if n == MAX_SHIFTS:
            raise CoderError("more than three byte moves in one step")
        move(low >> 24)
        low = (low << 8) & MASK
        rng = (rng << 8) & MASK
        n += 1


def encode(symbols):
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
        low, rng = _normalize(low, rng, out.append)
        n += 1
    if n:
        for _ in range(4):
            out.append(low >> 24)
            low = (low << 8) & MASK
    return bytes(out)


def decode(code, count, model):
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
        v = min(((c - low) & MASK) // rng, total - 1)
        sym, cum, freq = find(v)
        low = (low + cum * rng) & MASK
        rng = (freq * rng) & MASK

        def move(_byte):
            nonlocal c
            c = ((c << 8) | get()) & MASK

        low, rng = _normalize(low, rng, move)
        out.append(sym)
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
