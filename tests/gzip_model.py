"""Python model of the GZIP codec's frame (bitar_amd/cpp/src/gzip_frame.h) and of the
bit-granular join under it (bitar_amd/csrc/deflate_join.hip), with Python integers as the
bit buffer.  Shared by the CPU frame tests and the GPU tests."""
import struct
import zlib

STORED = 1 << 23
SEG = 65536


def model_join(slots, bits):
    """slots: the segments' raw DEFLATE streams (bytes; a coded one is ONE block, a stored one
    is one or two byte-aligned stored blocks), bits: their lengths in bits
    -> (joined stream, starts[nseg + 1])"""
    pos, acc, starts = 0, 0, []
    for i, (slot, nb) in enumerate(zip(slots, bits)):
        last = i == len(slots) - 1
        starts.append(pos)
        if slot[0] & 6:  # coded: one block
            v = int.from_bytes(slot, "little") & ((1 << nb) - 1)
            if not last:
                v &= ~1
            acc |= v << pos
            pos += nb
        else:  # stored
            two = len(slot) > 65540
            if last and not two:
                acc |= 1 << pos
            pos = (pos + 3 + 7) & ~7
            body = bytearray(slot[1:])
            if two:
                body[65539] = 1 if last else 0
            acc |= int.from_bytes(bytes(body), "little") << pos
            pos += 8 * (len(slot) - 1)
    starts.append(pos)
    return acc.to_bytes((pos + 7) // 8, "little"), starts


def index_starts(entries):
    """the same positions from the index alone (gzip_frame.h IndexStarts)"""
    pos, starts = 0, []
    for e in entries:
        starts.append(pos)
        nb = e & 0xFFFFF
        pos = ((pos + 3 + 7) & ~7) + nb - 8 if e & STORED else pos + nb
    starts.append(pos)
    return starts


def fixed_literal_block(data):
    """one final fixed-Huffman block of literals only -> (bytes, bits)"""
    acc, pos = 0b011, 3  # BFINAL = 1, BTYPE = 01

    def put(code, n):  # Huffman codes go most significant bit first
        nonlocal acc, pos
        for k in range(n - 1, -1, -1):
            acc |= ((code >> k) & 1) << pos
            pos += 1
    for b in data:
        if b < 144:
            put(0x30 + b, 8)
        else:
            put(0x190 + b - 144, 9)
    put(0, 7)  # end of block
    return acc.to_bytes((pos + 7) // 8, "little"), pos


def stored_segment(data):
    """ceil(n / 65535) stored blocks, the last one final -> (bytes, bits)"""
    out, p = bytearray(), 0
    nblk = max(1, (len(data) + 65534) // 65535)
    for b in range(nblk):
        chunk = data[p:p + 65535]
        out += struct.pack("<BHH", 1 if b + 1 == nblk else 0, len(chunk), len(chunk) ^ 0xFFFF)
        out += chunk
        p += len(chunk)
    return bytes(out), 8 * len(out)


def header(seg, entries, flg_extra=0, name=None, comment=None, hcrc=False, more_extra=b""):
    extra = b"BT" + struct.pack("<HII", 8 + 3 * len(entries), seg, len(entries))
    extra += b"".join(struct.pack("<I", e)[:3] for e in entries) + more_extra
    flg = 4 | flg_extra | (8 if name is not None else 0) | (16 if comment is not None else 0) \
        | (2 if hcrc else 0)
    h = bytes([0x1f, 0x8b, 8, flg, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", len(extra)) + extra
    if name is not None:
        h += name + b"\0"
    if comment is not None:
        h += comment + b"\0"
    if hcrc:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h


def indexed_member(data, seg, stored_every=0, **kw):
    """a member as the codec writes it, from CPU-made segment streams: fixed literal blocks,
    every stored_every-th segment stored -> (member bytes, expected table entry)"""
    slots, bits, entries = [], [], []
    for i in range(0, len(data), seg):
        piece = data[i:i + seg]
        st = stored_every and (i // seg) % stored_every == stored_every - 1
        s, nb = stored_segment(piece) if st else fixed_literal_block(piece)
        slots.append(s)
        bits.append(nb)
        entries.append(nb | (STORED if st else 0))
    if slots:
        stream, starts = model_join(slots, bits)
    else:
        stream, starts = b"\x03\x00", [0]
    h = header(seg, entries, **kw)
    member = h + stream + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)
    table = {"deflate_off": len(h), "deflate_len": len(stream), "csize": len(member),
             "crc": zlib.crc32(data), "isize": len(data), "indexed": 1, "seg": seg,
             "nseg": len(entries), "entries": entries, "starts": starts}
    return member, table


def plain_member_table(member, data, header_len=10):
    return {"deflate_off": header_len, "deflate_len": len(member) - header_len - 8,
            "csize": len(member), "crc": zlib.crc32(data), "isize": len(data), "indexed": 0,
            "seg": 0, "nseg": 0, "entries": [], "starts": []}


def bgzf(data, chunk=SEG - 256):
    """a BGZF file: one member per chunk, raw zlib DEFLATE, the 'BC' subfield = BSIZE;
    -> (file bytes, [table entries])"""
    out, tables = bytearray(), []
    pieces = [data[i:i + chunk] for i in range(0, len(data), chunk)] + [b""]  # + the EOF block
    for piece in pieces:
        c = zlib.compressobj(1, zlib.DEFLATED, -15)
        body = c.compress(piece) + c.flush()
        total = 18 + len(body) + 8
        h = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", 6) + b"BC" + \
            struct.pack("<HH", 2, total - 1)
        m = h + body + struct.pack("<II", zlib.crc32(piece), len(piece))
        t = plain_member_table(m, piece, 18)
        t["offset"] = len(out)
        tables.append(t)
        out += m
    return bytes(out), tables
