"""The BCF typed-walk table: one record per case, every count and descriptor written by hand (record_expect's builders).  Shared
by the host reader's test (test_decoder_edge_cases.py) and the device's (test_gpu_record_split_limits.py).

Header: vcf_bcf_writer.header_text(True, []) -- contigs "1", "2"; strings PASS, AF, DP, DB, CSQ, AC, MQS, TAGS.  Watched keys: one
of every kind the device decodes.  A case is (name, record, label); the label is written down here, from the format, and never
computed: DECIDED = a row, REJECT = refused by both readers, LIMIT = refused by the device layout alone (more than 8 FILTER
entries: the host reader decodes the record)."""
import struct

import record_expect as X

N_CONTIGS, N_STRINGS = 2, 8
AF, DP, DB, CSQ, AC, MQS, TAGS = range(1, 8)
KEYS = [(AF, "f"), (DP, "i"), (DB, "b"), (AC, "I"), (MQS, "F")]
INFO_FIELD = "AF,DP,DB,AC,MQS"
DECIDED, REJECT, LIMIT = "decided", "reject", "limit"
F1, F2 = 0x3F800000, 0x40490FDB  # 1.0f, pi
FILL = bytes([X.FILL])


def key(k):
    return X.typed_ints([k])


def good(i):
    """a well-formed record with a value under every watched key; i varies POS, QUAL, FILTER and the values"""
    info = [(key(AF), X.typed_floats([F1 + i])), (key(DP), X.typed_ints([1000 * i - 7])), (key(AC), X.typed_ints([i, None, 70000])),
            (key(MQS), X.typed_floats([F2, X.FLOAT_MISSING, F1 + i]))]
    if i % 2:
        info.insert(2, (key(DB), b"\x00"))
    return X.bcf_record(chrom=i % 2, pos0=i - 1, qual_bits=X.FLOAT_MISSING if i % 3 == 0 else F2 + i, id_=X.typed_str(b"rs%d" % i),
                        alleles=(X.typed_str(b"A"), X.typed_str(b"CT")), filter_=[b"\x00", X.typed_ints([0]), X.typed_ints([1, 2])][i % 3],
                        info=info)


# where a typed value can stand, with the item type that belongs there and a watched key for the INFO values
PLACES = {"id": 7, "allele": 7, "filter": 1, "key": 1, "val_f": 5, "val_i": 3, "val_b": 1, "val_I": 2, "val_F": 5}
VAL_KEY = {"val_f": AF, "val_i": DP, "val_b": DB, "val_I": AC, "val_F": MQS}


def items(t, n, first=1):
    """n items of type t as payload bytes: characters, small integers (valid FILTER indexes / key DP), floats"""
    if t == 7:
        return bytes(65 + (first + e) % 26 for e in range(n))
    if t == 5:
        return b"".join(struct.pack("<I", F1 + first + e) for e in range(n))
    return b"".join((1 + (first + e) % 6).to_bytes(X.TYPE_SIZE[t], "little") for e in range(n))


def place(where, value, behind_key=None, **kw):
    """a record with the typed value `value` at `where`, everything else well-formed"""
    if where == "id":
        return X.bcf_record(id_=value, info=[(key(AF), X.typed_floats([F2]))], pos0=41, **kw)
    if where == "allele":
        return X.bcf_record(alleles=(X.typed_str(b"G"), value), info=[(key(AF), X.typed_floats([F2]))], pos0=42, **kw)
    if where == "filter":
        return X.bcf_record(filter_=value, info=[(key(AF), X.typed_floats([F2]))], pos0=43, **kw)
    if where == "key":
        return X.bcf_record(info=[(value, X.typed_ints([77]) if behind_key is None else behind_key)], pos0=44, **kw)
    return X.bcf_record(info=[(key(DB), b"\x00"), (key(VAL_KEY[where]), value)], pos0=45, qual_bits=F1, **kw)


def cut_shared(rec, ls):
    """the record with its shared block cut to ls bytes (and nothing behind it)"""
    return struct.pack("<II", ls, 0) + rec[8:8 + ls]


def cases():
    out = []
    for where, t in PLACES.items():
        # extended counts for small vectors, in every width; 15 and 16 items (15 is the first count that needs the extended form)
        n_small = 1 if where == "key" else 3
        for cw in (1, 2, 3):
            out.append((f"{where}: {n_small} items, count as int{8 << (cw - 1) if cw < 3 else 32}",
                        place(where, X.typed(n_small, t, items(t, n_small), count_width=cw)), DECIDED))
        if where != "key":  # (a key is one integer)
            for n in (15, 16):
                out.append((f"{where}: {n} items", place(where, X.typed(n, t, items(t, n))), LIMIT if where == "filter" else DECIDED))
        # counts whose byte size wraps 32 bits: 2^30 four-byte items (0 mod 2^32), 2^31 - 1 two-byte items (-2), 2^31 - 1 bytes.
        # Eight bytes of payload follow, so a reader that stepped by the wrapped size would find a value there.  A key's count is
        # no length anybody steps by -- the key is the first integer -- so a huge count in front of an integer key is read, and
        # refused only where the type is no integer's
        for n, ht in ((0x40000000, 3), (0x40000000, 5), (0x7FFFFFFF, 2), (0x7FFFFFFF, 7)):
            if where == "key":
                rec = place(where, X.typed(n, ht, DP.to_bytes(X.TYPE_SIZE[ht], "little")))
                out.append((f"key: count {n:#x} of type {ht}", rec, DECIDED if ht in (2, 3) else REJECT))
            else:
                out.append((f"{where}: count {n:#x} of type {ht}", place(where, X.typed(n, ht, items(ht if ht != 2 else 1, 8))), REJECT))
        for n, cw in ((-1, 1), (-1, 3), (-(1 << 31), 3)):
            out.append((f"{where}: count {n} (width {cw})", place(where, X.typed(n, t, items(t, 4), count_width=cw)), REJECT))
        for cd in (0x15, 0x17, 0x10):
            out.append((f"{where}: count descriptor {cd:#x}", place(where, X.typed(0, t, items(t, 4), count_bytes=bytes([cd, 3, 0, 0, 0]))), REJECT))
        # the value ends exactly at l_shared / one byte beyond it.  Only a FILTER without INFO pairs and the last INFO value can be
        # the last thing in a well-formed shared block; behind an ID or an allele the next descriptor is missing
        value = key(DP) if where == "key" else X.typed(4, t, items(t, 4))
        rec = place(where, value, n_info=0) if where == "filter" else place(where, value)
        if where in ("id", "allele", "filter", "key"):
            full = cut_shared(rec, rec.index(value, 32) + len(value) - 8)
            label = DECIDED if where == "filter" else REJECT
        else:
            full, label = rec, DECIDED
        ls = struct.unpack_from("<I", full, 0)[0]
        out.append((f"{where}: ends at l_shared", full, label))
        out.append((f"{where}: ends one byte beyond l_shared", cut_shared(full, ls - 1), REJECT))
    out.append(("n_info larger than the pairs present", X.bcf_record(info=[(key(AF), X.typed_floats([F1]))], n_info=2), REJECT))
    out.append(("n_info larger than the pairs present, filler behind", X.bcf_record(info=[(key(AF), X.typed_floats([F1]))], n_info=3, tail=FILL * 2), REJECT))
    out.append(("l_shared = 24", cut_shared(X.bcf_record(), 24), REJECT))
    out.append(("FILTER of 8 entries", place("filter", X.typed_ints([0, 1, 2, 3, 4, 5, 6, 7])), DECIDED))
    out.append(("FILTER of 9 entries", place("filter", X.typed_ints([0, 1, 2, 3, 4, 5, 6, 7, 0])), LIMIT))
    out.append(("FILTER index n_strings - 1", place("filter", X.typed_ints([N_STRINGS - 1], width=2)), DECIDED))
    out.append(("FILTER index n_strings", place("filter", X.typed_ints([N_STRINGS], width=3)), REJECT))
    out.append(("FILTER index -3", place("filter", X.typed_ints([0, -3])), REJECT))
    out.append(("FILTER descriptor of type 7", place("filter", X.typed_str(b"\x01")), REJECT))
    out.append(("FILTER descriptor of type 5", place("filter", X.typed_floats([1])), REJECT))
    out.append(("CHROM n_contigs", X.bcf_record(chrom=N_CONTIGS), REJECT))
    out.append(("CHROM -1", X.bcf_record(chrom=-1), REJECT))
    for k, kind in KEYS:  # a watched key twice: the first occurrence wins
        a, b = {"f": (X.typed_floats([F1]), X.typed_floats([F2])), "i": (X.typed_ints([5]), X.typed_ints([600])),
                "b": (b"\x00", X.typed_ints([1])), "I": (X.typed_ints([1, 2]), X.typed_ints([3])),
                "F": (X.typed_floats([F1, F2]), X.typed_floats([F2]))}[kind]
        out.append((f"key of kind {kind} twice", X.bcf_record(info=[(key(k), a), (key(CSQ), X.typed_str(b"x")), (key(k), b)]), DECIDED))
        if kind != "b":  # (a first `key=.` is no value: the statement says what the second one then means)
            miss = X.typed_floats([X.FLOAT_MISSING]) if kind in "fF" else X.typed_ints([None])
            out.append((f"key of kind {kind} twice, the first missing", X.bcf_record(info=[(key(k), miss), (key(k), b)]), DECIDED))
    names = [c[0] for c in out]
    assert len(set(names)) == len(names)
    return out
