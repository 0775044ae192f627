"""The list chunks of a parquet file as arguments of tools/pq_list_fuzz.cpp:
offset:size:codec:type_size:leaf_level:max_def:slots:rows:raw_size per chunk.

    python tools/pq_list_fuzz_chunks.py FILE"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nvtabular_amd.parquet_plain import PlainParquetFile

pf = PlainParquetFile(sys.argv[1])
assert pf.readable, pf.why_not
out = []
for rg in pf.row_groups:
    for col, dt, cc in zip(pf.columns, pf.dtypes, rg["columns"]):
        if col["kind"] == "list" and rg["num_rows"]:
            out.append(":".join(str(int(v)) for v in (cc["offset"], cc["size"], cc["codec"], dt.itemsize, col["leaf_level"],
                                                       col["max_def"], cc["num_values"], rg["num_rows"], cc["raw_size"])))
print(" ".join(out))
