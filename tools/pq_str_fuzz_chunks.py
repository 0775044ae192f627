"""The string chunks of a parquet file as arguments of tools/pq_str_fuzz.cpp:
offset:size:codec:max_def:rows:raw_size per chunk.

    python tools/pq_str_fuzz_chunks.py FILE"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nvtabular_amd.parquet_plain import PlainParquetFile

pf = PlainParquetFile(sys.argv[1])
assert pf.decodable, pf.why_pyarrow
out = []
for rg in pf.row_groups:
    for col, cc in zip(pf.columns, rg["columns"]):
        if col["kind"] == "string" and rg["num_rows"]:
            out.append(":".join(str(int(v)) for v in (cc["offset"], cc["size"], cc["codec"], col["max_def"],
                                                       rg["num_rows"], cc["raw_size"])))
print(" ".join(out))
