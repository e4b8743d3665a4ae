#!/usr/bin/env python3
"""tools/sorted_info.py DB.jf -- the device memory `query -s` takes for a binary/sorted database, by both look-up paths: the
records as the file has them with their bucket index (jfgpu_sorted_create, then jfgpu_sorted_info) and a hash table of the
header's size (jfgpu_create, then jfgpu_get_info; the table the records are loaded into grows from there when it must).
One line each on stdout.  Needs a GPU.  tools/query_sorted_bench.sh calls it."""
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from jellyfish_amd import capi  # noqa: E402


def main(path):
    with open(path, "rb") as f:
        hlen = int(f.read(9))
        header = json.loads(f.read(hlen).rstrip(b"\0"))
    assert header["format"] == "binary/sorted", header["format"]
    k, vb, m = header["key_len"] // 2, header["counter_len"], header["matrix1"]
    cols = None if m.get("identity") else np.array(m["columns"], dtype=np.uint64)
    body = np.memmap(path, dtype=np.uint8, mode="r", offset=9 + hlen)
    with capi.Sorted(k, header["size"], cols, vb, body, canonical=bool(header["canonical"]), matrix_rows=m["r"]) as s:
        i = s.info()
    print("sorted_info k=%d records=%d bucket_bits=%d longest_bucket=%d device_bytes=%d upload_us=%d index_us=%d file_body_bytes=%d"
          % (k, i["n_records"], i["bucket_bits"], i["longest_bucket"], i["device_bytes"], i["upload_us"], i["index_us"], len(body)))
    try:
        with capi.Table(k, header["size"], canonical=bool(header["canonical"])) as t:
            print("table_info k=%d size=%d slot_bytes=%d table_bytes=%d" % (k, t.info.size, t.info.slot_bytes, t.info.table_bytes))
    except capi.JfgpuError as e:
        print("table_info k=%d size=%d not created: %s" % (k, header["size"], e.msg))


if __name__ == "__main__":
    main(sys.argv[1])
