"""Fuzzed FASTA for the tests of kr_batch_submit_fasta / kr_fasta_chunk_cut (no test of its own): records unwrapped or wrapped at
60, 7 or 1 columns, LF or CRLF per file, blank lines, blanks, tabs and control bytes in bodies, comments holding `> + @`, names
holding bytes >= 128, empty names, sometimes no final newline -- and, with probability p_bad per record, one of the corruptions
that must end the device's accepted prefix."""
import numpy as np

ALPHA = np.frombuffer(b"ACGTNacgtRYK", np.uint8)
HIGH = ["é", "ü", "Ω"]  # every byte of their UTF-8 forms is >= 128 (the reader's names are decoded as UTF-8)


def wrap_body(seq, wrap, nl):
    if wrap == 0 or not seq:
        return seq + nl
    return b"".join(seq[j:j + wrap] + nl for j in range(0, len(seq), wrap))


def insert(body, rng, what):
    at = int(rng.integers(0, len(body)))  # in front of a byte of the body, whose last byte is a newline: never in front of the next '>'
    return body[:at] + what + body[at:]


def fuzz_fasta(rng, n, p_bad, max_len=400):
    """n records; returns (bytes, start offset of every record written)"""
    nl = b"\r\n" if rng.random() < 1 / 3 else b"\n"
    out, starts, pos = [], [], 0
    for i in range(n):
        L = int(rng.integers(0, max_len + 1)) if rng.random() < 0.95 else 0
        seq = ALPHA[rng.integers(0, len(ALPHA), L)].tobytes()
        head = b">r%d_%d" % (i, int(rng.integers(0, 1 << 20)))
        hk = int(rng.integers(0, 7))
        if hk == 1:
            head += b" comment > with + and @"
        elif hk == 2:
            head += b"\tx"
        elif hk == 3:
            head = b">"
        elif hk == 4:
            head += HIGH[int(rng.integers(0, len(HIGH)))].encode()
        elif hk == 5:
            head = b"> nameless \xff comment"
        body = wrap_body(seq, int(rng.choice([0, 60, 7, 1])), nl)
        if rng.random() < 0.1:
            body += nl
        if rng.random() < 0.1:
            body = nl + body
        if rng.random() < 1 / 15:
            body = insert(body, rng, b" ")
        if rng.random() < 1 / 15:
            body = insert(body, rng, b"\t")
        if rng.random() < 1 / 20:
            body = insert(body, rng, bytes([127 if rng.random() < 0.5 else int(rng.integers(1, 9))]))
        if rng.random() < p_bad:
            kind = int(rng.integers(0, 8))
            if kind == 0:
                body = insert(body, rng, b"+")
            elif kind == 1:
                body = insert(body, rng, b"@")
            elif kind == 2:
                body = insert(body, rng, b">")
            elif kind == 3:
                body = b"+" + nl + body
            elif kind == 4:
                body = b"@x" + nl + body
            elif kind == 5:
                head, body = b"@q%d" % i, seq + b"\n+\n" + b"I" * len(seq) + b"\n"
            elif kind == 6:
                head = head[:1] + b"\0" + head[1:]
            else:
                body = insert(body, rng, bytes([int(rng.integers(128, 256))]))
        rec = head + (b"\n" if head.startswith(b"@") else nl) + body
        starts.append(pos)
        out.append(rec)
        pos += len(rec)
    raw = b"".join(out)
    if rng.random() < 1 / 3 and raw.endswith(b"\n"):
        raw = raw[:-1]
    return raw, starts


def records(capi, path, offset=None):
    """(names as bytes, sequences as bytes) from the project's sequential reader"""
    names, bases, offs = capi.read_fastx(path, offset=offset)
    return [x.encode() for x in names], [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(names))]
