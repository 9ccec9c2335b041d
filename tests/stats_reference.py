"""The pseudo-gradient statistics restated on the CPU (what edt_delta_stats must equal bit for bit;
DESIGN.md §3): torch computes d_k and the mean m with the reference's own loop in theta's dtype
(EDT_LM/diloco.py:243-246, `acc += (w - g) / K`), what is not finite is zeroed before the sums and
counted with isfinite, and oracle.canonical_chunk_sums forms {S_kk, S_mm, S_km} per chunk in the
documented order. Rows are laid out as the kernel's: S_mm | S_kk[K] | S_km[K] | nonfinite_mean |
nonfinite[K]; S_km is zero above 8 workers."""
import numpy as np
import torch


def make_chunks(seg_offsets, chunk_elems=1 << 16):
    """edt_slerp_make_chunks' table on the host: [nchunks, 3] = start, length, segment."""
    out = []
    for s, (a, b) in enumerate(zip(seg_offsets[:-1], seg_offsets[1:])):
        for x in range(a, b, chunk_elems):
            out.append((x, min(chunk_elems, b - x), s))
    return np.asarray(out, dtype=np.int64).reshape(-1, 3)


def deltas_and_mean(theta, workers):
    """(d [K tensors], m) in theta's dtype, torch CPU, the reference's loop."""
    g = theta.detach().cpu()
    K = len(workers)
    acc = torch.zeros_like(g)
    ds = []
    for w in workers:
        d = w.detach().cpu() - g              # promoted to theta's dtype (fp32 master, bf16 workers)
        assert d.dtype == g.dtype
        ds.append(d)
        acc += d / K
    return ds, acc


def stats_rows(theta, workers, chunks, oracle):
    """float64 [nchunks, 3 K + 2] and the rounded mean m."""
    K = len(workers)
    ds, m = deltas_and_mean(theta, workers)
    chunks = np.asarray(chunks, dtype=np.int64).reshape(-1, 3)
    rows = np.zeros((len(chunks), 3 * K + 2))
    mf = m.float()
    m_ok = torch.isfinite(mf)
    mz = torch.where(m_ok, mf, torch.zeros_like(mf))

    def count(ok):
        bad = (~ok).numpy().astype(np.int64)
        return np.asarray([bad[a:a + n].sum() for a, n, _ in chunks], dtype=np.float64)

    rows[:, 2 * K + 1] = count(m_ok)
    for k, d in enumerate(ds):
        df = d.float()
        ok = torch.isfinite(df)
        dz = torch.where(ok, df, torch.zeros_like(df))
        s = oracle.canonical_chunk_sums(dz, mz, chunks)
        rows[:, 1 + k] = s[:, 0]
        rows[:, 0] = s[:, 1]
        if K <= 8:
            rows[:, 1 + K + k] = s[:, 2]
        rows[:, 2 * K + 2 + k] = count(ok)
    return rows, m


def same_bits(a, b) -> bool:
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
    b = np.ascontiguousarray(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def operands(n, K, gdt, wdt, seed, scale=0.02):
    """theta and K workers (CPU) with signed zeros and subnormals planted among normal values."""
    gen = torch.Generator().manual_seed(seed)
    theta = (torch.randn(n, generator=gen) * 0.5).to(gdt)
    workers = [(theta.float() + torch.randn(n, generator=gen) * scale).to(wdt) for _ in range(K)]
    specials = [0.0, -0.0, 1e-40, -1e-40, 3e-39]
    for j, v in enumerate(specials):
        if n > 3 * j + 2:
            theta[3 * j] = v                         # base special, workers normal
            workers[j % K][3 * j + 1] = v            # one worker special
            theta[3 * j + 2] = v                     # both: a zero / subnormal delta
            workers[(j + 1) % K][3 * j + 2] = -v if j % 2 else v
    return theta, workers
