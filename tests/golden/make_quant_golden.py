#!/usr/bin/env python3
"""Regenerates the encoder-quantisation fixtures (needs the reference sources and oracle/_ref).

quant_tables_encoder.json -- schro_table_quant, schro_table_offset_1_2, schro_table_offset_3_8 and
    schro_table_inverse_quant: the NUMBERS held by the reference's schrotables.c (read as text).  Data, no source: four
    lists of 61 integers.
quant_ref_digests.json -- for every quant index 0 .. 60 x {inter, intra}: all 65 536 s16 values through the Orc program
    schro_frame_data_quantise (schroencoder.c:3485-3553) picks for that index, called in oracle/_ref/libschroorc_ref.so
    with that function's arguments; one SHA-256 of the quantised array and one of the reconstructed array (the arrays
    themselves would be 32 MB).  Plus orc_subtract_s16 / orc_subtract_s16_u8 on fixed seeded rows.
"""
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
import quant_ref as Q  # noqa: E402

REF_TABLES = os.path.join(os.environ.get("REFERENCE", "/root/reference"), "schroedinger", "schrotables.c")
TABLE_NAMES = ("schro_table_quant", "schro_table_offset_1_2", "schro_table_offset_3_8", "schro_table_inverse_quant")


def main():
    src = open(REF_TABLES).read()

    def table(name):
        body = re.search(name + r"\[61\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
        return [int(v.rstrip("u")) for v in re.findall(r"\d+u?", body)]
    with open(Q.TABLES_PATH, "w") as f:
        json.dump({n: table(n) for n in TABLE_NAMES}, f)
        f.write("\n")
    assert O.ref_available(), "recording needs oracle/_ref"
    out = {}
    for intra in (0, 1):
        for qi in range(61):
            q, r = Q.quantise_s16_orc(Q.all_s16(), qi, intra)
            out["q%02d_%s" % (qi, "intra" if intra else "inter")] = {"quant": Q.sha(q), "recon": Q.sha(r)}
    for u8 in (0, 1):
        out["subtract_%s" % ("u8" if u8 else "s16")] = Q.sha(Q.subtract_orc(*Q.subtract_pin_inputs(u8)))
    with open(os.path.join(HERE, "quant_ref_digests.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
