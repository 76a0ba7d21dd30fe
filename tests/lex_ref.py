"""CPU restatement of the keyword (BM25) search, written from the scoring definition (DESIGN.md "Keyword search"),
not from the native code: ``re`` + ``zlib`` for the analyzer, ``math.log`` for idf, Python floats (IEEE fp64, one
rounding per operation) for every term contribution and Python ints for the fixed-point sum.  The GPU results must
equal these bit for bit."""
import math
import re
import zlib

TERM_BITS = 22
MAX_QTERMS = 64
_TOKEN = re.compile(r"[\u4e00-\u9fff]|[^\W\u4e00-\u9fff]+|[^\w\s]")


def analyze(text):
    """Term ids of a text, in token order."""
    return [zlib.crc32(t.encode("utf-8")) % (1 << TERM_BITS) for t in _TOKEN.findall(text.lower())]


def pack_row(tokens):
    """(entries, dl) of one row: distinct terms ascending as ``term << 10 | min(count, 1023)``, dl = min(len, 65535)."""
    counts = {}
    for t in tokens:
        counts[t] = counts.get(t, 0) + 1
    return [(t << 10) | min(c, 1023) for t, c in sorted(counts.items())], min(len(tokens), 65535)


def pack(token_lists):
    """(entries, CSR offsets, dl) of several rows."""
    entries, offsets, dls = [], [0], []
    for tokens in token_lists:
        e, dl = pack_row(tokens)
        entries += e
        offsets.append(len(entries))
        dls.append(dl)
    return entries, offsets, dls


def round_half_even(x):
    """llrint of a non-negative double in the default rounding mode."""
    return round(x)  # Python's round(float) is exact round-half-to-even to an int


class RefIndex:
    """Rows of raw token-id lists; ``live[r]`` False = removed."""

    def __init__(self):
        self.rows = []   # per row: ({term: tf}, dl)
        self.live = []

    def add(self, token_lists):
        first = len(self.rows)
        for tokens in token_lists:
            e, dl = pack_row(tokens)
            self.rows.append(({x >> 10: x & 1023 for x in e}, dl))
            self.live.append(True)
        return first

    def remove(self, rows):
        for r in rows:
            self.live[r] = False

    def stats(self):
        """(N, sum_dl, df dict) over the live rows."""
        n, sum_dl, df = 0, 0, {}
        for (terms, dl), live in zip(self.rows, self.live):
            if live:
                n += 1
                sum_dl += dl
                for t in terms:
                    df[t] = df.get(t, 0) + 1
        return n, sum_dl, df

    def search(self, query_terms, k, allowed=None, k1=1.2, b=0.75):
        """Per query (a list of term ids): (scores, rows), k long, (score desc, row asc), -inf / -1 padding.
        ``allowed``: per-row booleans (None: every row)."""
        n, sum_dl, df = self.stats()
        out_s, out_r = [], []
        for q in query_terms:
            terms = [t for t in sorted(set(q))[:MAX_QTERMS] if df.get(t, 0) > 0]
            hits = []
            if terms:
                avgdl = sum_dl / n
                A = {}
                for t in terms:
                    idf = math.log(1.0 + (n - df[t] + 0.5) / (df[t] + 0.5))
                    A[t] = idf * (k1 + 1.0)
                for r, ((row_terms, dl), live) in enumerate(zip(self.rows, self.live)):
                    if not live or (allowed is not None and not allowed[r]):
                        continue
                    K = k1 * ((1.0 - b) + b * (dl / avgdl))
                    fixed, matched = 0, False
                    for t in terms:
                        tf = row_terms.get(t)
                        if tf is None:
                            continue
                        matched = True
                        c = (A[t] * tf) / (tf + K)
                        fixed += round_half_even(c * 4294967296.0)
                    if matched:
                        hits.append((-(fixed / 4294967296), r))  # exact: fixed < 2**53
            hits.sort()
            hits = hits[:k]
            out_s.append([-s for s, _ in hits] + [float("-inf")] * (k - len(hits)))
            out_r.append([r for _, r in hits] + [-1] * (k - len(hits)))
        return out_s, out_r
