"""tools/gen_random_reads.py OUT N_READS LENGTH SEED -- a FASTA of uniform random reads (numpy, seeded), for tools/merge_bench.sh."""
import sys
import numpy as np
out, n_reads, L, seed = sys.argv[1], int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4])
rng = np.random.default_rng(seed)
lut = np.frombuffer(b"ACGT", dtype=np.uint8)
with open(out, "wb") as f:
    done = 0
    while done < n_reads:
        n = min(200000, n_reads - done)
        rec = np.empty((n, L + 4), dtype=np.uint8)
        rec[:, 0] = ord(">"); rec[:, 1] = ord("r"); rec[:, 2] = ord("\n"); rec[:, -1] = ord("\n")
        rec[:, 3:-1] = lut[rng.integers(0, 4, (n, L), dtype=np.uint8)]
        f.write(rec.tobytes())
        done += n
