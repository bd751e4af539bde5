"""The files the tests of `zot scan` hand to the command: FASTA files of a case's records and k-mer sets of its samples."""
import numpy as np


def write_fasta(tmp_path, case):
    paths = []
    for k, recs in enumerate(case["fasta"]):
        paths.append(str(tmp_path / ("%s_%d.fa" % (case["name"], k))))
        with open(paths[-1], "w") as f:
            for nm, seq in recs:
                f.write(">%s\n" % nm)
                for at in range(0, len(seq), 60):
                    f.write(seq[at:at + 60] + "\n")
    return paths


def write_set(path, Kset, acgt, X):
    from zotmer_amd.library import vectors
    from zotmer_amd.library.container import KmerSet
    with KmerSet(str(path), "w") as z:
        vectors.write_kmers_and_counts(z, np.array(X, dtype=np.uint64), np.ones(len(X), dtype=np.uint64))
        z.meta.update({"K": Kset, "kmers": "kmers", "counts": "counts", "acgt": acgt})
    return str(path)
