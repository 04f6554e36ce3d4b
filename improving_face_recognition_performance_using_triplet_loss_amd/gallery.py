"""FaceGallery: enrolled face features resident on the device, searched 1:N by the gallery kernels (csrc/efm_gallery.hip).

The deployment side of the reference keeps enrolled features in SQLite / Postgres and scans them row by row on the CPU
(Feature.hpp:295-343 top-k rows, 345-392 argmax, 763-804 best identity).  Here the rows live in device memory, unit-norm, in the
gallery layout of include/efm_hip.h (fp32 or bf16, row stride pad32(d), zero pad columns), split into chunks below 2 GiB each;
`search` scans every chunk into one workspace and merges once, so no score matrix is ever formed.  Selection rule: rows scoring
>= sim_th, best score first, ties to the lower row; empty slots are index -1, score -inf, label -1.
"""
import numpy as np
import torch

from . import ops

CHUNK_BYTES = 1 << 31   # every chunk stays below the project's per-tensor limit
MIN_ROWS = 1024          # first allocation of a chunk


class FaceGallery:
    """Enrolled features of dimension d, stored as "bf16" or "f32" on `device`."""

    def __init__(self, d, dtype="bf16", device="cuda", chunk_rows=None):
        if dtype not in ("bf16", "f32"):
            raise ValueError("dtype must be 'bf16' or 'f32', got %r" % (dtype,))
        if not 1 <= int(d) <= 1024:
            raise ValueError("feature dimension d = %r outside 1..1024" % (d,))
        self.d = int(d)
        self.dtype = dtype
        self.device = torch.device(device)
        self.ld = ops.pad32(self.d)
        self.torch_dtype = torch.bfloat16 if dtype == "bf16" else torch.float32
        esize = 2 if dtype == "bf16" else 4
        max_rows = (CHUNK_BYTES - 1) // (self.ld * esize)
        self.chunk_rows = int(min(chunk_rows, max_rows) if chunk_rows else max_rows)
        if self.chunk_rows < 1:
            raise ValueError("chunk_rows must be >= 1")
        self._chunks = []       # [(rows tensor (capacity, ld), rows used)]
        self._labels = torch.empty((0,), dtype=torch.int32, device=self.device)
        self._n = 0
        self._ws = None

    def __len__(self):
        return self._n

    @property
    def capacity(self):
        return sum(c.shape[0] for c, _ in self._chunks)

    @property
    def chunks(self):
        """(rows tensor, rows used) per chunk: views of the device storage, in enrolment order."""
        return [(c[:used], used) for c, used in self._chunks]

    @property
    def labels(self):
        return self._labels[:self._n]

    def _grow_labels(self, need):
        if self._labels.numel() >= need:
            return
        cap = max(need, 2 * self._labels.numel(), MIN_ROWS)
        new = torch.empty((cap,), dtype=torch.int32, device=self.device)
        new[:self._n] = self._labels[:self._n]
        self._labels = new

    def _room(self):
        """The chunk with free rows (grown geometrically up to chunk_rows, or a new one) -> its list position."""
        if self._chunks:
            buf, used = self._chunks[-1]
            if used < buf.shape[0]:
                return len(self._chunks) - 1
            if buf.shape[0] < self.chunk_rows:
                new = torch.empty((min(2 * buf.shape[0], self.chunk_rows), self.ld), dtype=self.torch_dtype, device=self.device)
                new[:used] = buf[:used]
                self._chunks[-1] = (new, used)
                return len(self._chunks) - 1
        cap = min(MIN_ROWS, self.chunk_rows)
        self._chunks.append((torch.empty((cap, self.ld), dtype=self.torch_dtype, device=self.device), 0))
        return len(self._chunks) - 1

    def enroll(self, features, labels):
        """Append rows: features (m, d) float32 on the gallery's device, any norm; labels m ints (identity of each row)."""
        if not torch.is_tensor(features) or features.dim() != 2 or features.shape[1] != self.d or features.dtype != torch.float32:
            raise ValueError("features must be a (m, %d) float32 tensor" % self.d)
        if features.device != self.device and not (self.device.index is None and features.device.type == self.device.type):
            raise ValueError("features live on %s, the gallery on %s" % (features.device, self.device))
        features = features.contiguous()
        m = features.shape[0]
        lab = torch.as_tensor(np.asarray(labels.cpu() if torch.is_tensor(labels) else labels).reshape(-1).astype(np.int64))
        if lab.numel() != m:
            raise ValueError("%d labels for %d feature rows" % (lab.numel(), m))
        if m and (int(lab.min()) < -2 ** 31 or int(lab.max()) >= 2 ** 31):
            raise ValueError("labels must fit in int32")
        self._grow_labels(self._n + m)
        self._labels[self._n:self._n + m] = lab.to(torch.int32).to(self.device)
        done = 0
        while done < m:
            c = self._room()
            buf, used = self._chunks[c]
            take = min(m - done, buf.shape[0] - used)
            ops.gallery_pack(features[done:done + take], buf[used:used + take])
            self._chunks[c] = (buf, used + take)
            done += take
            self._n += take

    def _workspace(self, nbytes):
        if self._ws is None or self._ws.numel() * 4 < nbytes:
            self._ws = torch.empty(((nbytes + 3) // 4,), dtype=torch.float32, device=self.device)
        return self._ws

    def search(self, query, k=1, sim_th=-1.0, by_identity=False):
        """query (nq, d) float32 -> (scores, index, label), each (nq, k): the k best rows (by_identity: the k best distinct
        identities, each at its best row) scoring >= sim_th.  index -1 = no match (score -inf, label -1)."""
        if not isinstance(k, (int, np.integer)) or not 1 <= k <= ops.GALLERY_KMAX:
            raise ValueError("k = %r outside 1..%d" % (k, ops.GALLERY_KMAX))
        sim_th = float(sim_th)
        if sim_th != sim_th:
            raise ValueError("sim_th is NaN")
        if not torch.is_tensor(query) or query.dim() != 2 or query.shape[1] != self.d or query.dtype != torch.float32:
            raise ValueError("query must be a (nq, %d) float32 tensor" % self.d)
        query = query.contiguous()
        nq = query.shape[0]
        if nq == 0 or self._n == 0:
            return (torch.full((nq, k), -float("inf"), device=query.device), torch.full((nq, k), -1, dtype=torch.int32, device=query.device),
                    torch.full((nq, k), -1, dtype=torch.int32, device=query.device))
        used = [(buf, n) for buf, n in self._chunks if n > 0]
        ws = self._workspace(ops.gallery_workspace_bytes(nq, len(used), k))
        row0 = 0
        for slot, (buf, n) in enumerate(used):
            ops.gallery_scan(query, buf, n, self._labels[row0:row0 + n] if by_identity else None, row0, k, sim_th, ws, slot)
            row0 += n
        scores, index, label = ops.gallery_merge(ws, len(used), nq, k, by_identity)
        if not by_identity:  # row mode: the label of each returned row (bookkeeping; the selection is the kernels')
            label = torch.where(index >= 0, self._labels[index.clamp(min=0).long()], torch.full_like(index, -1))
        return scores, index, label

    def features(self):
        """All enrolled rows as stored (unit norm), as a float32 (n, d) tensor."""
        parts = [buf[:n, :self.d].float() for buf, n in self._chunks if n > 0]
        return torch.cat(parts) if parts else torch.empty((0, self.d), dtype=torch.float32, device=self.device)

    def save(self, path):
        """.npz of the stored features (float32, unit norm) and labels: loads into a gallery of either dtype."""
        np.savez(path, features=self.features().cpu().numpy(), labels=self.labels.cpu().numpy().astype(np.int32))

    @classmethod
    def load(cls, path, dtype="bf16", device="cuda", chunk_rows=None):
        z = np.load(path)
        feats, labels = z["features"], z["labels"]
        g = cls(feats.shape[1], dtype=dtype, device=device, chunk_rows=chunk_rows)
        if feats.shape[0]:
            g.enroll(torch.as_tensor(feats, dtype=torch.float32).to(g.device), labels)
        return g

