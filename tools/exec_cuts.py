"""Diagnostic: per SF1 column, the batches k_snappy_exec5's producer cuts and why each one ends,
with the fixed far-copy slots (24 copies a batch, 80 bytes read per copy) and with far sources packed by
16-byte chunk (X5_FCH chunks a batch, only the chunks that cover a source are read).

batches() replays exec5_piece's producer over one 64 KiB piece's tokens: the 1 KiB input chunks, the cuts
(128 tokens, X5_BATCH = 764 bytes, a literal longer than 64 bytes alone, a literal not staged, the far limit,
the landed frontier LF from the batch history) and the empty batches (R5_NOP) a far copy waits through when it
is a batch's first token. One assumption: a source's address is taken as congruent to its output offset
modulo 16 (the arenas' and pages' real alignment is not known here), which fixes fsh.

    python tools/exec_cuts.py [rows] [X5_FCH] [column,column,...]
"""
import collections
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

X5_BATCH, TOKS, XRING, XSLOT, XCHUNK, XFAR, LINE, BLOCK = 764, 128, 4096, 1024, 1024, 24, 128, 65536
X5_FCH = 64
# why a batch ended (its last token is followed by a token that could not join it)
REASONS = ("far", "chunks", "tokens", "bytes", "long", "frontier", "input", "end")


def nchunks(addr, ol):
    """Aligned 16-byte chunks covering [addr, addr + ol)."""
    return ((addr & 15) + ol + 15) >> 4


def batches(toks, out_start, out_end, packed, fch=X5_FCH, xfar=XFAR, addr0=0):
    """The producer's batches of one piece. toks: [(in_pos, kind, ol, off, tl)] in stream order (kind 0 a
    literal, else a copy), the first one starting at output offset out_start. packed: chunk-packed far sources,
    else the fixed slots. addr0: address of output offset 0 (only its low 4 bits matter).
    Returns [(kind, reason, tokens, bytes, far copies, far chunks)], kind "normal" / "long" / "nop" / "bad"."""
    out = []
    op, i, ip = out_start, 0, toks[0][0] if toks else 0
    ops_m1, k_m1, k_m2, nops = out_start, "nop", "nop", 0
    T_end = 0   # tokens [i, T_end) are enumerated (the current input chunk)
    I = 0
    while op < out_end and i < len(toks):
        sf = out_start + ((ops_m1 - out_start) & ~(XSLOT - 1))
        LF = (sf - XSLOT if sf >= out_start + XSLOT else out_start) if k_m2 == "normal" else sf
        if i >= T_end:   # next input chunk: tokens starting in [ip, I + XCHUNK)
            I = toks[i][0] & ~15
            T_end = i
            while T_end < len(toks) and toks[T_end][0] < I + XCHUNK:
                T_end += 1
        b_op = op
        j, tot, nfar, nch_tot, reason = i, 0, 0, 0, None
        first_fnr = False
        while True:
            if j >= len(toks) or op + tot >= out_end:
                reason = "end"
                break
            if j >= T_end:
                reason = "input"
                break
            if j - i >= TOKS:
                reason = "tokens"
                break
            pos, kind, ol, off, tl = toks[j]
            otok = op + tot
            if ol > 64 or (kind == 0 and pos + tl > I + XCHUNK + 64):   # (a literal not staged whole)
                reason = "long"
                break
            if tot + ol > X5_BATCH:
                reason = "bytes"
                break
            a = otok - off
            far = kind != 0 and a + min(ol, off) <= op and a - (op + X5_BATCH - XRING) < 0
            if far:
                if packed:
                    n = nchunks(addr0 + a, ol)
                    fnr = a + ol + LINE - 1 > LF   # (the loads end at or below a + ol + 15, their line 112 bytes on)
                    if nch_tot + n > fch:
                        reason = "chunks"
                        break
                else:
                    n = 5
                    fnr = a + 80 + LINE > LF
                    if nfar >= xfar:
                        reason = "far"
                        break
                if fnr:
                    reason = "frontier"
                    first_fnr = j == i
                    break
                nfar += 1
                nch_tot += n
            tot += ol
            j += 1
        if j == i:   # no token could be taken
            pos, kind, ol, off, tl = toks[i]
            if kind == 0:
                rec = ("long", "long", 1, ol, 0, 0)
                op += ol
                i += 1
                nops = 0
            elif first_fnr and nops < 3:
                rec = ("nop", "frontier", 0, 0, 0, 0)
                nops += 1
            else:
                out.append(("bad", reason, 0, 0, 0, 0))
                break
        else:
            rec = ("normal", reason, j - i, tot, nfar, nch_tot)
            op += tot
            i = j
            nops = 0
        out.append(rec)
        k_m2, k_m1, ops_m1 = k_m1, rec[0], b_op
    return out


def far_chunk_need(toks, out_start, addr0=0):
    """(far copies, chunks that cover them) of a piece, far taken against the token's own position."""
    op, nf, nc = out_start, 0, 0
    for pos, kind, ol, off, tl in toks:
        if kind != 0 and off > XRING and off >= ol:
            nf += 1
            nc += nchunks(addr0 + op - off, ol)
        op += ol
    return nf, nc


def summarize(recs):
    st = collections.Counter()
    for kind, reason, nt, nb, nf, nc in recs:
        st["batches"] += 1
        st[kind] += 1
        if kind == "normal":
            st["cut_" + reason] += 1
        elif kind == "nop":
            st["cut_frontier_nop"] += 1
    return st


def page_pieces(stream):
    """{piece: [(in_pos, kind, ol, off, tl)]} of one raw Snappy stream, by the 64 KiB block a token starts in."""
    from snappy_stats import tokens
    out, pieces = 0, collections.defaultdict(list)
    for t in tokens(stream):
        pieces[out >> 16].append(t)
        out += t[2]
    return pieces, out


def fmt(st):
    n = max(st["batches"], 1)
    cuts = " ".join(f"{r} {st['cut_' + r]}" for r in REASONS if st["cut_" + r])
    return (f"batches {st['batches']:7d} (normal {st['normal']}, long {st['long']}, nop {st['nop']}, bad {st['bad']}) "
            f"far-limit share {100.0 * (st['cut_far'] + st['cut_chunks']) / n:5.1f}% | {cuts}")


def main():
    import numpy as np
    sys.path[:0] = [os.path.join(ROOT, "parquet-floor_amd"), os.path.join(ROOT, "tools")]
    import pyarrow.parquet as pq
    from pfloor import datagen
    from pfloor.decoder import ParquetFile

    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 1 << 20
    fch = int(sys.argv[2]) if len(sys.argv) > 2 else X5_FCH
    only = set(sys.argv[3].split(",")) if len(sys.argv) > 3 else None
    path = f"/tmp/probe_lineitem_{rows}.parquet"
    if not os.path.exists(path):
        pq.write_table(datagen.lineitem_table(rows, seed=42), path, compression="snappy", row_group_size=1 << 20)
    print(f"# {rows} rows, one row group; X5_FCH {fch}; per column: pieces, then the fixed slots, then packed chunks")
    with ParquetFile(path) as pf:
        names = [f.name for f in pq.ParquetFile(path).schema_arrow]
        for col in range(pf.num_columns):
            if only and names[col] not in only:
                continue
            s, n = pf.chunk_range(0, col)
            buf = np.zeros(n, np.uint8)
            pf.read_into(s, n, buf.ctypes.data)
            d = pf.chunk_desc(0, col, 0)
            old, new = collections.Counter(), collections.Counter()
            npieces = nfar = nchk = 0
            for i in range(d.n_pages):
                pg = d.pages[i]
                if pg.compressed_size >= pg.uncompressed_size:
                    continue
                pieces, total = page_pieces(buf[pg.offset:pg.offset + pg.compressed_size].tobytes())
                if sum(len(v) for v in pieces.values()) <= 1:   # one literal: read in place, no executor
                    continue
                for k, tl in pieces.items():
                    lo, hi = k * BLOCK, min((k + 1) * BLOCK, total)
                    npieces += 1
                    old.update(summarize(batches(tl, lo, hi, False)))
                    new.update(summarize(batches(tl, lo, hi, True, fch)))
                    f, c = far_chunk_need(tl, lo)
                    nfar += f
                    nchk += c
            if not npieces:
                continue
            print(f"{names[col]:16s} pieces {npieces:4d} | batches a piece {old['batches'] / npieces:7.1f} -> "
                  f"{new['batches'] / npieces:7.1f} ({100.0 * (new['batches'] - old['batches']) / max(old['batches'], 1):+5.1f}%) | "
                  f"far copies {nfar:7d}, chunks needed per far copy {nchk / max(nfar, 1):4.2f} | frontier cuts "
                  f"{old['cut_frontier'] + old['nop']} -> {new['cut_frontier'] + new['nop']}", flush=True)
            print(f"    slots : {fmt(old)}")
            print(f"    packed: {fmt(new)}", flush=True)


if __name__ == "__main__":
    main()
