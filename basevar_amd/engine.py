"""Host-side mirror of the reference's per-site interface, batched.

The reference calls, once per genomic site (src/basetype_caller.cpp:742-743, 1113-1164):

    BaseType bt(&batchinfo, min_af);  bt.lrt();
    bt.get_alt_bases(); bt.get_lrt_af(b); bt.get_var_qual(); bt.get_total_depth(); bt.get_base_depth(b)
    strand_bias(ref, alts, bases, strands);  ref_vs_alt_ranksumtest(ref, alts, bases, values)

``BaseTypeEngine.lrt(slab)`` does all of that for every site (row) of a slab in one submit
through the C ABI (include/basevar_amd.h) and returns ``BaseTypeBatch``, whose getters carry
the reference's names and take the site index as first argument.  Errors the reference
raises as std::runtime_error surface as RuntimeError with the same message.

torch is used only for device memory and streams; it never appears in the ABI.
"""
import ctypes as C

import numpy as np

from . import _capi

BASES = "ACGT"  # src/basetype.h:19


def min_af(n_samples, user_min_af=0.01):  # noqa: D401
    """(double)std::min(float(100)/n, min_af): src/basetype_caller.cpp:122."""
    return _capi.load().bv_min_af(int(n_samples), float(user_min_af))


class BaseTypeBatch:
    """Per-site records of one submit (numpy structured arrays on the host)."""

    def __init__(self, sites, groups, n_variant, pass1_ms, pass2_ms):
        self.sites = sites
        self.groups = groups
        self.n_variant = n_variant
        self.pass1_ms = pass1_ms
        self.pass2_ms = pass2_ms

    # --- BaseType getters, src/basetype.h:121-151
    def get_alt_bases(self, i):
        r = self.sites[i]
        return [BASES[b] for b in r["alt"][:r["n_alt"]]]

    def get_lrt_af(self, i, b):
        r = self.sites[i]
        alts = [BASES[x] for x in r["alt"][:r["n_alt"]]]
        if b not in alts:  # std::map::at -> out_of_range -> runtime_error, basetype.h:141-149
            raise RuntimeError("[ERROR] out_of_range:: map::at '%s' not found." % b)
        return float(r["af"][alts.index(b)])

    def get_var_qual(self, i):
        return float(self.sites[i]["qual"])

    def get_total_depth(self, i):
        return int(self.sites[i]["total_depth"])

    def get_base_depth(self, i, b):
        if b not in BASES:
            raise RuntimeError("[ERROR] out_of_range:: map::at '%s' not found." % b)
        return float(self.sites[i]["depth"][BASES.index(b)])

    # --- StrandBiasInfo of the two strand_bias() calls, src/basetype.h:57-62
    def strand_bias(self, i, flavour="vcf"):
        r = self.sites[i]
        k = "var" if flavour == "vcf" else "cvg"
        sb = r[k + "_sb"]
        return {"ref_fwd": int(sb[0]), "ref_rev": int(sb[1]), "alt_fwd": int(sb[2]), "alt_rev": int(sb[3]),
                "fs": float(r[k + "_fs"]), "sor": float(r[k + "_sor"])}

    # --- the three ref_vs_alt_ranksumtest() values; the reference truncates them to int
    def rank_sums(self, i):
        r = self.sites[i]
        return float(r["mq_ranksum"]), float(r["rpr_ranksum"]), float(r["bq_ranksum"])


class BaseTypeEngine:
    """One engine per GPU / host thread (mirrors one BaseType per ThreadPool worker)."""

    def __init__(self, max_sites, min_af_value, device=0, flags=0, max_samples=0):
        self._lib = _capi.load()
        cfg = _capi.EngineConfig(int(device), int(max_sites), int(max_samples), int(flags), float(min_af_value))
        h = C.c_void_p()
        rc = self._lib.bv_engine_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise RuntimeError("bv_engine_create failed (%d): %s" % (rc, self._lib.bv_last_error(None).decode()))
        self._h = h
        self.device = int(device)
        self.max_sites = int(max_sites)
        self.min_af = float(min_af_value)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.bv_engine_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _err(self):
        return self._lib.bv_last_error(self._h).decode()

    # ---- raw pointer interface (device or host pointers as ints)
    def submit_ptrs(self, n_sites, n_samples, pitch, base_strand, qual, ref_base, out, mapq=0, rpr=0, group_id=0,
                    n_groups=0, gout=0, mem_kind=_capi.BV_MEM_DEVICE, stream=0, layout=0):
        """`layout`: bv_slab.layout (BV_SLAB_RPR_TAGGED: the rpr plane carries the cells' calls, include/basevar_amd.h)."""
        slab = _capi.Slab(int(n_sites), int(n_samples), int(pitch), base_strand or None, qual or None, mapq or None,
                          rpr or None, ref_base or None, group_id or None, int(n_groups), int(mem_kind), int(layout))
        rc = self._lib.bv_engine_submit(self._h, C.byref(slab), out or None, gout or None, stream or None)
        if rc != 0:
            raise RuntimeError("bv_engine_submit failed (%d): %s" % (rc, self._err()))

    def submit_many_ptrs(self, n_samples, pitch, slabs, stream=0, group_id=0, n_groups=0, gouts=None, layout=0):
        """Several device-resident slabs as ONE launch per pass (bv_engine_submit_many / _g).  `slabs`: a sequence of
        (n_sites, base_strand, qual, ref_base, out, mapq, rpr) with device pointers as ints (mapq = rpr = 0: no rank sums);
        pop-groups: one `group_id` array for the whole queue, `gouts[k]` = slab k's group records."""
        n = len(slabs)
        arr = (_capi.Slab * n)()
        outs = (C.c_void_p * n)()
        gp = (C.c_void_p * n)() if n_groups else None
        for k, (n_sites, bs, q, ref, out, mq, rp) in enumerate(slabs):
            arr[k] = _capi.Slab(int(n_sites), int(n_samples), int(pitch), bs or None, q or None, mq or None, rp or None, ref or None,
                                group_id or None, int(n_groups), _capi.BV_MEM_DEVICE, int(layout))
            outs[k] = out
            if n_groups:
                gp[k] = gouts[k]
        rc = self._lib.bv_engine_submit_many_g(self._h, n, arr, outs, gp, stream or None)
        if rc != 0:
            raise RuntimeError("bv_engine_submit_many failed (%d): %s" % (rc, self._err()))

    def join(self, stream=0):
        """Make `stream` wait for every submit issued so far (needed with BV_FLAG_LANES: bv_engine_join)."""
        if self._lib.bv_engine_join(self._h, C.c_void_p(stream) if stream else None) != 0:
            raise RuntimeError("bv_engine_join: " + self._err())

    def stream_handle(self):
        """hipStream_t of the engine's own stream as an int (e.g. for torch.cuda.ExternalStream).  The stream dies with the
        engine: free torch tensors that were used on it -- pinned host blocks above all, whose allocator records an event on
        every stream a block has seen when the block is freed -- before close()."""
        return int(self._lib.bv_engine_stream(self._h) or 0)

    def wait(self):
        rc = self._lib.bv_engine_wait(self._h)
        if rc == _capi.BV_ERR_SITE:
            raise RuntimeError(self._err())  # the reference's runtime_error text, basetype.cpp:114
        if rc != 0:
            raise RuntimeError("bv_engine_wait failed (%d): %s" % (rc, self._err()))

    def kernel_ms(self):
        a, b = C.c_float(), C.c_float()
        rc = self._lib.bv_engine_kernel_ms(self._h, C.byref(a), C.byref(b))
        if rc != 0:
            raise RuntimeError("bv_engine_kernel_ms failed (%d): %s" % (rc, self._err()))
        return a.value, b.value

    def timing_reset(self):
        if self._lib.bv_engine_timing_reset(self._h) != 0:
            raise RuntimeError("bv_engine_timing_reset: " + self._err())

    def timing_get(self):
        """(total pass-1 ms, total pass-2 ms, number of submits) since timing_reset()."""
        a, b, n = C.c_double(), C.c_double(), C.c_uint32()
        if self._lib.bv_engine_timing_get(self._h, C.byref(a), C.byref(b), C.byref(n)) != 0:
            raise RuntimeError("bv_engine_timing_get: " + self._err())
        return a.value, b.value, n.value

    def timing_get_ex(self):
        """(streaming-kernel ms, pass-1 ms, pass-2 ms, submits) since timing_reset(); on short rows pass 1 is the
        streaming kernel plus the solve kernel, on long rows it is one kernel and the first two figures coincide."""
        s, a, b, n = C.c_double(), C.c_double(), C.c_double(), C.c_uint32()
        if self._lib.bv_engine_timing_get_ex(self._h, C.byref(s), C.byref(a), C.byref(b), C.byref(n)) != 0:
            raise RuntimeError("bv_engine_timing_get_ex: " + self._err())
        return s.value, a.value, b.value, n.value

    @property
    def host_log_exact(self):
        """True when shallow sites are replayed with the host libm's own log() (verified bit-exact at creation)."""
        return bool(self._lib.bv_engine_host_log_exact(self._h))

    def host_log_eval(self, x):
        """The device restatement of the host's log() at the float64 array x (diagnostic)."""
        import numpy as np
        x = np.ascontiguousarray(x, dtype=np.float64)
        y = np.empty_like(x)
        if self._lib.bv_engine_host_log_eval(self._h, x.ctypes.data, y.ctypes.data, x.size) != 0:
            raise RuntimeError("bv_engine_host_log_eval: " + self._err())
        return y

    def last_launch_form(self):
        """BV_FORM_* bits of the last launch's pass 1 (include/basevar_amd_diag.h)."""
        f = C.c_uint32()
        if self._lib.bv_engine_last_launch_form(self._h, C.byref(f)) != 0:
            raise RuntimeError("bv_engine_last_launch_form: " + self._err())
        return f.value

    def last_variant_count(self):
        n = C.c_uint32()
        self._lib.bv_engine_last_variant_count(self._h, C.byref(n))
        return n.value

    # ---- sample-axis tile mode (numpy tiles in host memory)
    def lrt_tiles(self, slab, tile_width, max_rank=0, packed=False, sparse_batch=0):
        """`packed`: every tile goes as its covered cells only (bv_engine_tiles_add_sparse: 7 bytes per covered cell, one packed
        host allocation per tile); a number k > 1: every k-th tile dense, the others packed (a job may mix the two).
        `sparse_batch` k > 0: the packed tiles go in calls of k (bv_engine_tiles_add_sparse_many; fewer before a dense tile
        and at the end); 0: one bv_engine_tiles_add_sparse per packed tile.
        Same result as lrt(slab), but the slab is fed as column tiles of `tile_width` samples
        (the reference's `-B/--batch-count` batchfiles) that the engine accumulates in HBM.  Every tile is one packed
        host allocation (bv_tile_packed_layout), so it crosses the link as one copy.  `max_rank`: an upper bound on the
        read-position ranks, for the per-site-tally realisation (see bv_engine_tiles_begin)."""
        bs = np.ascontiguousarray(slab["base_strand"], dtype=np.uint8)
        S = bs.shape[0]
        N = int(slab.get("n_samples", bs.shape[1]))
        q = np.asarray(slab["qual"], dtype=np.uint8)
        mq, rp = slab.get("mapq"), slab.get("rpr")
        ranks = mq is not None and rp is not None
        gid = slab.get("group_id")
        ng = int(slab.get("n_groups", 0)) if gid is not None else 0
        ref = np.ascontiguousarray(slab["ref_base"], dtype=np.uint8)
        rc = self._lib.bv_engine_tiles_begin(self._h, S, N, ng, (max(2, int(max_rank)) if max_rank else 1) if ranks else 0)
        if rc != 0:
            raise RuntimeError("bv_engine_tiles_begin failed (%d): %s" % (rc, self._err()))
        keep = []  # the copies are asynchronous: every tile stays alive until the final wait
        lay = int(slab.get("layout", 0))
        pending = []  # sparse_batch: packed tiles not sent yet

        def flush():
            if pending:
                self.tiles_add_sparse_many(pending)
                del pending[:]
                if len(keep) >= 64:  # every tile held has been handed over: bound the host memory held by tiles in flight
                    self.wait()
                    del keep[:]
        for k_tile, lo in enumerate(range(0, N, tile_width)):
            w = min(tile_width, N - lo)
            if packed and not (packed > 1 and k_tile % int(packed) == 0):
                # the tile's covered cells, site after site (np.nonzero walks row-major: sites in order, samples ascending)
                cb = bs[:, lo:lo + w]
                rows, cols = np.nonzero(cb != 8)
                E = int(rows.size)
                offs = (C.c_uint64 * 7)()
                total = C.c_uint64()
                rc = self._lib.bv_sparse_tile_packed_layout(S, E, w, 1 if ranks else 0, 1 if ng else 0, offs, C.byref(total))
                if rc != 0:
                    raise RuntimeError("bv_sparse_tile_packed_layout failed (%d)" % rc)
                buf = np.zeros(total.value + 256, dtype=np.uint8)
                pad = (-buf.ctypes.data) % 256

                def arr(kk, dt, n):
                    return buf[pad + offs[kk]: pad + offs[kk] + n * np.dtype(dt).itemsize].view(dt)
                rs = arr(0, np.uint32, S + 1); rs[0] = 0; rs[1:] = np.cumsum(np.bincount(rows, minlength=S))
                a_s = arr(1, np.uint16, E); a_s[:] = cols
                a_b = arr(2, np.uint8, E); a_b[:] = cb[rows, cols]
                a_q = arr(3, np.uint8, E); a_q[:] = q[:, lo:lo + w][rows, cols]
                a_m = a_r = a_g = None
                if ranks:
                    a_m = arr(4, np.uint8, E); a_m[:] = np.asarray(mq)[:, lo:lo + w][rows, cols]
                    a_r = arr(5, np.uint16, E); a_r[:] = np.asarray(rp)[:, lo:lo + w][rows, cols] & (0x1FFF if lay & 1 else 0xFFFF)  # plain ranks
                if ng:
                    a_g = arr(6, np.uint8, w); a_g[:] = np.asarray(gid, dtype=np.uint8)[lo:lo + w]
                keep.append(buf)
                p = lambda a: None if a is None else a.ctypes.data
                t = _capi.SparseTile(S, w, E, ng, p(rs), p(a_s), p(a_b), p(a_q), p(a_m), p(a_r), p(a_g), _capi.BV_MEM_HOST, lay)
                if sparse_batch:
                    pending.append(t)
                    if len(pending) >= int(sparse_batch):
                        flush()
                    continue
                rc = self._lib.bv_engine_tiles_add_sparse(self._h, C.byref(t), None)
                if rc != 0:
                    raise RuntimeError("bv_engine_tiles_add_sparse failed (%d): %s" % (rc, self._err()))
                if len(keep) >= 64:
                    self.wait()
                    del keep[:-1]
                continue
            flush()  # (the packed tiles before this dense one go first)
            pitch, total = C.c_uint64(), C.c_uint64()
            offs = (C.c_uint64 * 5)()
            rc = self._lib.bv_tile_packed_layout(S, w, 1 if ranks else 0, 1 if ng else 0, C.byref(pitch), offs, C.byref(total))
            if rc != 0:
                raise RuntimeError("bv_tile_packed_layout failed (%d)" % rc)
            P = pitch.value
            buf = np.zeros(total.value + 256, dtype=np.uint8)
            base = buf.ctypes.data
            pad = (-base) % 256  # 256-byte aligned start inside the numpy allocation

            def plane(k, dt, rows, fill):
                n = rows * P * np.dtype(dt).itemsize
                v = buf[pad + offs[k]: pad + offs[k] + n].view(dt).reshape(rows, P)
                v[...] = fill
                return v
            tb = plane(0, np.uint8, S, 8); tb[:, :w] = bs[:, lo:lo + w]
            tq = plane(1, np.uint8, S, 0); tq[:, :w] = q[:, lo:lo + w]
            tm = tr = tg = None
            if ranks:
                tm = plane(2, np.uint8, S, 0); tm[:, :w] = np.asarray(mq)[:, lo:lo + w]
                tr = plane(3, np.uint16, S, 0); tr[:, :w] = np.asarray(rp)[:, lo:lo + w]
            if ng:
                tg = plane(4, np.uint8, 1, 0xFF); tg[0, :w] = np.asarray(gid, dtype=np.uint8)[lo:lo + w]
            keep.append(buf)
            p = lambda a: None if a is None else a.ctypes.data
            t = _capi.Slab(S, w, P, p(tb), p(tq), p(tm), p(tr), None, p(tg), ng, _capi.BV_MEM_HOST, int(slab.get("layout", 0)))
            rc = self._lib.bv_engine_tiles_add(self._h, C.byref(t), None)
            if rc != 0:
                raise RuntimeError("bv_engine_tiles_add failed (%d): %s" % (rc, self._err()))
            if len(keep) >= 64:  # bound the host memory held by in-flight tiles
                self.wait()
                del keep[:-1]
        flush()
        out = np.zeros(S, dtype=_capi.SITE_DTYPE)
        gout = np.zeros((S, ng), dtype=_capi.GROUP_DTYPE) if ng else None
        rc = self._lib.bv_engine_tiles_finish(self._h, ref.ctypes.data, out.ctypes.data,
                                              gout.ctypes.data if ng else None, _capi.BV_MEM_HOST, None)
        if rc != 0:
            raise RuntimeError("bv_engine_tiles_finish failed (%d): %s" % (rc, self._err()))
        self.wait()
        return BaseTypeBatch(out, gout, self.last_variant_count(), 0.0, 0.0)

    def tiles_add_many(self, tiles, stream=0):
        """tiles: list of _capi.Slab (one open tile job, bv_engine_tiles_begin): device-resident tiles of a joined-rows job go
        to their columns in one launch per 256 tiles (bv_engine_tiles_add_many)."""
        arr = (_capi.Slab * len(tiles))(*tiles)
        rc = self._lib.bv_engine_tiles_add_many(self._h, len(tiles), arr, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise RuntimeError("bv_engine_tiles_add_many failed (%d): %s" % (rc, self._err()))

    def tiles_add_sparse_many(self, tiles, stream=0):
        """tiles: list of _capi.SparseTile (one open tile job): n calls of bv_engine_tiles_add_sparse as one call
        (bv_engine_tiles_add_sparse_many): one staging copy set and one launch per group of tiles.  Host tiles must stay
        untouched until wait()."""
        arr = (_capi.SparseTile * len(tiles))(*tiles)
        rc = self._lib.bv_engine_tiles_add_sparse_many(self._h, len(tiles), arr, C.c_void_p(stream) if stream else None)
        if rc != 0:
            raise RuntimeError("bv_engine_tiles_add_sparse_many failed (%d): %s" % (rc, self._err()))

    # ---- numpy slab (host memory; the engine stages it to HBM)
    def lrt(self, slab):
        """slab: dict of numpy planes as produced by basevar_amd.synth.make_slab()."""
        bs = np.ascontiguousarray(slab["base_strand"], dtype=np.uint8)
        S, pitch = bs.shape
        N = int(slab.get("n_samples", pitch))
        q = np.ascontiguousarray(slab["qual"], dtype=np.uint8)
        mq = slab.get("mapq")
        rp = slab.get("rpr")
        mq = None if mq is None else np.ascontiguousarray(mq, dtype=np.uint8)
        rp = None if rp is None else np.ascontiguousarray(rp, dtype=np.uint16)
        ref = np.ascontiguousarray(slab["ref_base"], dtype=np.uint8)
        gid = slab.get("group_id")
        ng = int(slab.get("n_groups", 0)) if gid is not None else 0
        gid = None if gid is None else np.ascontiguousarray(gid, dtype=np.uint8)
        out = np.zeros(S, dtype=_capi.SITE_DTYPE)
        gout = np.zeros((S, ng), dtype=_capi.GROUP_DTYPE) if ng else None
        p = lambda a: 0 if a is None else a.ctypes.data
        self.submit_ptrs(S, N, pitch, p(bs), p(q), p(ref), p(out), p(mq), p(rp), p(gid), ng, p(gout),
                         mem_kind=_capi.BV_MEM_HOST, layout=int(slab.get("layout", 0)))
        self.wait()
        ms1, ms2 = self.kernel_ms()
        return BaseTypeBatch(out, gout, self.last_variant_count(), ms1, ms2)

    # ---- batchfile text rows, parsed on the device
    def lrt_text(self, rows, file_samples, group_id=None, n_groups=0, host_reader=None, tokens="host"):
        """The reference's own batchfile rows in, records out (bv_engine_text_parse + bv_engine_text_submit).

        `rows`: one list per position of its row in every batchfile (bytes, without the line break), or a packed pair
        (text, row_off) -- text bytes / uint8 array, row_off uint64 [n_positions * n_files + 1], every row ending in b"\n".
        `file_samples`: samples per batchfile.  The device parses every position in the strict form of a well-formed row;
        any other position comes back BV_TEXT_HOST and goes to `host_reader(list of row bytes) -> (cell, phred, mapq, rank,
        ref_code)` numpy rows of n_samples, or None for a skipped position; without a host_reader such a position raises.
        Returns a TextBatch: the records (one per position not skipped), `positions` (their indices), `row_state`
        [n_positions][n_files] and the returned `cell` / `phred` planes [records][n_samples].  The engine must have been
        created with max_samples >= sum(file_samples).  `tokens`: "host" (the default) leaves the '+SEQ' / '-SEQ' tokens of the
        marked rows to the caller; "device" lists them on the device during the parse (text_tokens_enable for this call) and
        the batch carries `tokens` / `token_text` as text_tokens_fetch returns them."""
        restore = self._tokens_mode(tokens, "lrt_text")
        try:
            return self._lrt_text(rows, file_samples, group_id, n_groups, host_reader, tokens == "device")
        finally:
            restore()

    def _tokens_mode(self, tokens, who):
        """tokens="device": the mode on for one call; returns what puts it back"""
        if tokens not in ("host", "device"):
            raise ValueError("%s: tokens is 'host' or 'device'" % who)
        was = getattr(self, "_text_tokens_on", False)
        if tokens == "device" and not was:
            self.text_tokens_enable(True)
            return lambda: self.text_tokens_enable(False)
        return lambda: None

    def _lrt_text(self, rows, file_samples, group_id, n_groups, host_reader, device_tokens):
        fs = np.ascontiguousarray(file_samples, dtype=np.uint32)
        F, N = int(fs.size), int(fs.sum())
        text, off, P = self._pack_rows(rows, F, "lrt_text")
        gid = None if group_id is None else np.ascontiguousarray(group_id, dtype=np.uint8)
        tr = _capi.TextRows(text.ctypes.data, off.ctypes.data, fs.ctypes.data, int(text.size), int(P), F, 0)
        state = np.zeros((P, F), dtype=np.uint8)
        rc = self._lib.bv_engine_text_parse(self._h, C.byref(tr), None if gid is None else gid.ctypes.data, int(n_groups),
                                            state.ctypes.data, None)
        if rc != 0:
            raise RuntimeError("bv_engine_text_parse failed (%d): %s" % (rc, self._err()))
        batch = self._text_submit("lrt_text", state, P, F, N, n_groups, host_reader,
                                  lambda p: [bytes(text[int(off[p * F + f]):int(off[p * F + f + 1]) - 1]) for f in range(F)])
        if device_tokens:
            batch.tokens, batch.token_text = self.text_tokens_fetch()
        return batch

    def _text_submit(self, what, state, P, F, N, n_groups, host_reader, lines_of):
        """the host positions of a parsed batch through host_reader, then bv_engine_text_submit: a TextBatch"""
        host = []
        for p in np.nonzero(state[:, 0] & _capi.BV_TEXT_HOST)[0]:
            if host_reader is None:
                raise RuntimeError("%s: position %d is not in the strict form the device parses and no host_reader was given" % (what, p))
            lines = lines_of(int(p))
            got = host_reader(lines)
            if got is None:
                state[p, :] = _capi.BV_TEXT_SKIP
            else:
                host.append(got)
        positions = np.nonzero((state[:, 0] & _capi.BV_TEXT_SKIP) == 0)[0].astype(np.uint32)
        R = int(positions.size)
        hs = None
        keep = []
        if host:
            pitch = (N + 15) // 16 * 16
            planes = [np.full((len(host), pitch), 8, np.uint8), np.zeros((len(host), pitch), np.uint8),
                      np.zeros((len(host), pitch), np.uint8), np.zeros((len(host), pitch), np.uint16)]
            ref = np.zeros(len(host), np.uint8)
            for h, (cell, phred, mapq, rank, ref_code) in enumerate(host):
                for k, v in enumerate((cell, phred, mapq, rank)):
                    planes[k][h, :N] = v
                ref[h] = ref_code
            keep = planes + [ref]
            hs = _capi.Slab(len(host), N, pitch, *[a.ctypes.data for a in planes[:2]], planes[2].ctypes.data, planes[3].ctypes.data,
                            ref.ctypes.data, None, 0, _capi.BV_MEM_HOST, 0, 0)
        out = np.zeros(R, dtype=_capi.SITE_DTYPE)
        gout = np.zeros((R, n_groups), dtype=_capi.GROUP_DTYPE) if n_groups else None
        cell = np.zeros((R, N), np.uint8)
        phred = np.zeros((R, N), np.uint8)
        rc = self._lib.bv_engine_text_submit(self._h, state.ctypes.data, C.byref(hs) if hs is not None else None, int(P),
                                             out.ctypes.data, gout.ctypes.data if n_groups else None, cell.ctypes.data,
                                             phred.ctypes.data, None)
        del keep
        if rc != 0:
            raise RuntimeError("bv_engine_text_submit failed (%d): %s" % (rc, self._err()))
        n_variant = 0
        if R:
            self.wait()
            n_variant = self.last_variant_count()
        return TextBatch(out, gout, n_variant, positions, state, cell, phred)

    # ---- batchfile text rows, parsed a few files at a time (include/basevar_amd_text_job.h)
    @staticmethod
    def _pack_rows(rows, F, who):
        """rows of lrt_text -> (text uint8, row_off uint64, P)"""
        if isinstance(rows, tuple):
            text, off = rows
            text = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, np.uint8)
            off = np.ascontiguousarray(off, dtype=np.uint64)
            return text, off, (off.size - 1) // F
        if any(len(pos) != F for pos in rows):
            raise ValueError("%s: every position needs one row per batchfile" % who)
        flat = [bytes(r) + b"\n" for pos in rows for r in pos]
        off = np.zeros(len(flat) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(r) for r in flat])
        return np.frombuffer(b"".join(flat), dtype=np.uint8), off, len(rows)

    def text_job_begin(self, n_positions, file_samples, group_id=None, n_groups=0):
        """bv_engine_text_job_begin: a parse job of n_positions x len(file_samples) rows"""
        fs = np.ascontiguousarray(file_samples, dtype=np.uint32)
        gid = None if group_id is None else np.ascontiguousarray(group_id, dtype=np.uint8)
        rc = self._lib.bv_engine_text_job_begin(self._h, int(n_positions), int(fs.size), fs.ctypes.data, None if gid is None else gid.ctypes.data,
                                                int(n_groups), None)
        if rc != 0:
            raise RuntimeError("bv_engine_text_job_begin failed (%d): %s" % (rc, self._err()))

    def text_job_add(self, rows, file_samples, first_file, want_flags=True):
        """bv_engine_text_job_add: the rows of files [first_file, first_file + len(file_samples)), as lrt_text takes rows.
        Returns the add's BV_TEXT_INDEL marks [n_positions][files of the add] (None without want_flags)."""
        fs = np.ascontiguousarray(file_samples, dtype=np.uint32)
        K = int(fs.size)
        text, off, P = self._pack_rows(rows, K, "text_job_add")
        tr = _capi.TextRows(text.ctypes.data, off.ctypes.data, fs.ctypes.data, int(text.size), int(P), K, 0)
        flags = np.zeros((P, K), dtype=np.uint8) if want_flags else None
        rc = self._lib.bv_engine_text_job_add(self._h, C.byref(tr), int(first_file), flags.ctypes.data if want_flags else None, None)
        if rc != 0:
            raise RuntimeError("bv_engine_text_job_add failed (%d): %s" % (rc, self._err()))
        return flags

    def text_job_finish(self, n_positions, n_files):
        """bv_engine_text_job_finish: row_state [n_positions][n_files] of the whole job"""
        state = np.zeros((int(n_positions), int(n_files)), dtype=np.uint8)
        rc = self._lib.bv_engine_text_job_finish(self._h, state.ctypes.data, None)
        if rc != 0:
            raise RuntimeError("bv_engine_text_job_finish failed (%d): %s" % (rc, self._err()))
        return state

    def lrt_text_job(self, adds, file_samples, group_id=None, n_groups=0, host_reader=None, tokens="host"):
        """lrt_text with the files delivered in groups (bv_engine_text_job_begin / _add / _finish + bv_engine_text_submit).

        `adds`: a list of (first_file, rows) in any file order; `rows` as lrt_text takes them, for the adjacent files
        first_file .. first_file + K, K being the rows per position (list form) -- a packed pair is given as
        (first_file, (text, row_off), K).  Every file of `file_samples` is added exactly once.  Returns what lrt_text returns
        for the rows of all files joined position-major; host_reader gets a host position's rows of all files, in file order."""
        restore = self._tokens_mode(tokens, "lrt_text_job")
        try:
            fs = np.ascontiguousarray(file_samples, dtype=np.uint32)
            F, N = int(fs.size), int(fs.sum())
            packed = []
            for add in adds:
                first, rows = int(add[0]), add[1]
                K = int(add[2]) if len(add) > 2 else (len(rows[0]) if len(rows) else 0)
                if K <= 0 or first < 0 or first + K > F:
                    raise ValueError("lrt_text_job: an add of files %d .. %d does not lie in the %d files" % (first, first + K, F))
                packed.append((first, K) + self._pack_rows(rows, K, "lrt_text_job"))
            if not packed:
                raise ValueError("lrt_text_job: no add")
            P = packed[0][4]
            self.text_job_begin(P, fs, group_id, n_groups)
            where = {}  # file -> (text, row_off, K, k): the host reader's lines come from the adds' own rows
            for first, K, text, off, _ in packed:
                self.text_job_add((text, off), fs[first:first + K], first, want_flags=False)
                for k in range(K):
                    where[first + k] = (text, off, K, k)
            state = self.text_job_finish(P, F)

            def lines_of(p):
                out = []
                for f in range(F):
                    text, off, K, k = where[f]
                    out.append(bytes(text[int(off[p * K + k]):int(off[p * K + k + 1]) - 1]))
                return out
            batch = self._text_submit("lrt_text_job", state, P, F, N, n_groups, host_reader, lines_of)
            if tokens == "device":
                batch.tokens, batch.token_text = self.text_tokens_fetch()
            return batch
        finally:
            restore()

    # ---- batchfile rows that are still compressed: inflated, split into lines and parsed on the device
    def lrt_bgzf(self, runs, file_samples, skip_bytes=None, skip_lines=None, max_positions=None, at_end=True, group_id=None, n_groups=0,
                 host_reader=None, tokens="host", region=None):
        """lrt_text for rows that are still BGZF members (bv_engine_text_parse_bgzf + bv_engine_text_rows_fetch +
        bv_engine_text_submit).  `runs`: per batchfile the list of its consecutive whole members (bytes) from where its next row
        starts; that row begins skip_bytes[f] inflated bytes into the run and skip_lines[f] lines further.  Takes
        min(max_positions, max_sites, the files' complete lines) positions; `at_end`: the runs reach the ends of their files.
        Returns what lrt_text returns plus `cursors` [n_files][2] -- (member of the run, inflated offset inside it) of every
        file's first line not taken -- and `fetched` = (bytes, row_off): the text the host needs (bv_engine_text_rows_fetch).
        A damaged member raises RuntimeError with `.args[1] == BV_ERR_DATA`.  `tokens`: as lrt_text's; with "device", `fetched` comes
        from text_heads_fetch (a marked row is cut like any other) and the batch carries `tokens` / `token_text`.
        `region` = (name, beg, end), 1-based inclusive: the rows are the region's lines (bv_engine_text_parse_bgzf_region,
        include/basevar_amd_region.h) -- lines in front of it are consumed, POS is held equal across the files -- and the batch
        carries `region_done` as well; a malformed head, files that disagree on the region's lines or on POS raise RuntimeError
        with `.args[1] == BV_ERR_DATA`.  Without `region`, exactly the calls above."""
        restore = self._tokens_mode(tokens, "lrt_bgzf")
        try:
            return self._lrt_bgzf(runs, file_samples, skip_bytes, skip_lines, max_positions, at_end, group_id, n_groups, host_reader, tokens == "device", region)
        finally:
            restore()

    def _lrt_bgzf(self, runs, file_samples, skip_bytes, skip_lines, max_positions, at_end, group_id, n_groups, host_reader, device_tokens, region=None):
        fs = np.ascontiguousarray(file_samples, dtype=np.uint32)
        F, N = int(fs.size), int(fs.sum())
        if len(runs) != F:
            raise ValueError("lrt_bgzf: one run per batchfile")
        members = [bytes(m) for run in runs for m in run]
        data = np.frombuffer(b"".join(members), dtype=np.uint8)
        moff = np.zeros(len(members) + 1, dtype=np.uint64)
        moff[1:] = np.cumsum([len(m) for m in members])
        fm = np.zeros(F + 1, dtype=np.uint32)
        fm[1:] = np.cumsum([len(run) for run in runs])
        sb = np.zeros(F, np.uint64) if skip_bytes is None else np.ascontiguousarray(skip_bytes, dtype=np.uint64)
        sl = np.zeros(F, np.uint32) if skip_lines is None else np.ascontiguousarray(skip_lines, dtype=np.uint32)
        cap = self.max_sites if max_positions is None else min(int(max_positions), self.max_sites)
        br = _capi.BgzfRows(data.ctypes.data if data.size else None, moff.ctypes.data, int(data.size), fm.ctypes.data, fs.ctypes.data, sb.ctypes.data,
                            sl.ctypes.data, F, self.max_sites if max_positions is None else int(max_positions), 1 if at_end else 0, 0)
        gid = None if group_id is None else np.ascontiguousarray(group_id, dtype=np.uint8)
        state = np.zeros((max(cap, 1), F), dtype=np.uint8)
        n_pos = C.c_uint32(0)
        cursors = np.zeros((F, 2), dtype=np.uint32)
        done = C.c_uint32(0)
        if region is None:
            rc = self._lib.bv_engine_text_parse_bgzf(self._h, C.byref(br), None if gid is None else gid.ctypes.data, int(n_groups), C.byref(n_pos),
                                                     state.ctypes.data, cursors.ctypes.data, None)
            if rc != 0:
                raise RuntimeError("bv_engine_text_parse_bgzf failed (%d): %s" % (rc, self._err()), rc)
        else:
            name = None if region[0] is None else (region[0].encode() if isinstance(region[0], str) else bytes(region[0]))
            rg = _capi.TextRegion(name, len(name) if name else 0, int(region[1]), int(region[2]), int(region[3]) if len(region) > 3 else 0)
            rc = self._lib.bv_engine_text_parse_bgzf_region(self._h, C.byref(br), C.byref(rg), None if gid is None else gid.ctypes.data, int(n_groups),
                                                            C.byref(n_pos), state.ctypes.data, cursors.ctypes.data, C.byref(done), None)
            if rc != 0:
                raise RuntimeError("bv_engine_text_parse_bgzf_region failed (%d): %s" % (rc, self._err()), rc)
        P = int(n_pos.value)
        state = np.ascontiguousarray(state.reshape(-1)[:P * F].reshape(P, F))
        if P == 0:
            batch = TextBatch(np.zeros(0, _capi.SITE_DTYPE), np.zeros((0, n_groups), _capi.GROUP_DTYPE) if n_groups else None, 0,
                              np.zeros(0, np.uint32), state, np.zeros((0, N), np.uint8), np.zeros((0, N), np.uint8))
            batch.cursors, batch.fetched = cursors, (np.zeros(0, np.uint8), np.zeros(1, np.uint64))
            if device_tokens:
                batch.tokens, batch.token_text = np.zeros(0, _capi.PILEUP_TOKEN_DTYPE), np.zeros(0, np.uint8)
            if region is not None:
                batch.region_done = bool(done.value)
            return batch
        fetched = self.text_heads_fetch(P * F) if device_tokens else self.text_rows_fetch(P * F)
        buf, roff = fetched
        batch = self._text_submit("lrt_bgzf", state, P, F, N, n_groups, host_reader,
                                  lambda p: [bytes(buf[int(roff[p * F + f]):int(roff[p * F + f + 1])]) for f in range(F)])
        batch.cursors, batch.fetched = cursors, fetched
        if device_tokens:
            batch.tokens, batch.token_text = self.text_tokens_fetch()
        if region is not None:
            batch.region_done = bool(done.value)
        return batch

    def text_rows_fetch(self, n_rows, capacity=None):
        """(bytes uint8, row_off uint64 [n_rows + 1]) of bv_engine_text_rows_fetch after a parse of n_rows rows; with `capacity`
        below what is needed: (None, bytes needed)"""
        return self._rows_fetch("bv_engine_text_rows_fetch", n_rows, capacity)

    def text_heads_fetch(self, n_rows, capacity=None):
        """text_rows_fetch with every BV_TEXT_INDEL row cut like any other parsed row (bv_engine_text_heads_fetch); refused after a
        parse that listed no tokens (text_tokens_enable), since the marked rows' tokens would be nowhere."""
        return self._rows_fetch("bv_engine_text_heads_fetch", n_rows, capacity)

    # ---- the '+SEQ' / '-SEQ' tokens of parsed rows, listed on the device (include/basevar_amd_text_tokens.h)
    def text_tokens_enable(self, on=True):
        """The mode for this engine's later parses (bv_engine_text_tokens_enable); the default is off."""
        rc = self._lib.bv_engine_text_tokens_enable(self._h, 1 if on else 0)
        if rc != 0:
            raise RuntimeError("bv_engine_text_tokens_enable failed (%d): %s" % (rc, self._err()), rc)
        self._text_tokens_on = bool(on)

    def text_tokens(self):
        """The last parse's tokens where they lie (bv_engine_text_tokens): ((device pointer, n_tokens), (device pointer,
        text_bytes)), what indel_tally(key, tokens=..., text=...) takes as device tokens; pos is the position's index."""
        T = _capi.IndelTokens()
        rc = self._lib.bv_engine_text_tokens(self._h, C.byref(T))
        if rc != 0:
            raise RuntimeError("bv_engine_text_tokens failed (%d): %s" % (rc, self._err()), rc)
        return (int(T.tokens or 0), int(T.n_tokens)), (int(T.text or 0), int(T.text_bytes))

    def text_tokens_fetch(self):
        """The last parse's tokens in host memory (bv_engine_text_tokens_fetch): (PILEUP_TOKEN_DTYPE array, uint8 text)."""
        n, nb = C.c_uint64(0), C.c_uint64(0)
        rc = self._lib.bv_engine_text_tokens_fetch(self._h, None, 0, None, 0, C.byref(n), C.byref(nb), None)  # no room: the sizes
        if rc != 0 and not (rc == _capi.BV_ERR_INVALID_ARG and n.value):
            raise RuntimeError("bv_engine_text_tokens_fetch failed (%d): %s" % (rc, self._err()), rc)
        tok = np.zeros(int(n.value), dtype=_capi.PILEUP_TOKEN_DTYPE)
        text = np.zeros(int(nb.value), dtype=np.uint8)
        if tok.size:
            rc = self._lib.bv_engine_text_tokens_fetch(self._h, tok.ctypes.data, int(tok.size), text.ctypes.data, int(text.size), C.byref(n), C.byref(nb), None)
            if rc != 0:
                raise RuntimeError("bv_engine_text_tokens_fetch failed (%d): %s" % (rc, self._err()), rc)
        return tok, text

    def _rows_fetch(self, symbol, n_rows, capacity):
        need = C.c_uint64(0)
        roff = np.zeros(int(n_rows) + 1, dtype=np.uint64)
        if capacity is None:
            rc = getattr(self._lib, symbol)(self._h, None, 0, roff.ctypes.data, C.byref(need), None)
            if rc != 0:
                raise RuntimeError("%s failed (%d): %s" % (symbol, rc, self._err()))
            capacity = int(need.value)
        buf = np.zeros(max(int(capacity), 1), dtype=np.uint8)
        rc = getattr(self._lib, symbol)(self._h, buf.ctypes.data, int(capacity), roff.ctypes.data, C.byref(need), None)
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (symbol, rc, self._err()))
        if int(need.value) > int(capacity):
            return None, int(need.value)
        return buf[:int(need.value)], roff

    # ---- BGZF members, inflated on the device
    def bgzf_inflate(self, members_bytes, member_off, dst_ptr=0, dst_capacity=0):
        """Whole BGZF members as they lie in a file in, their inflated bytes out (bv_engine_bgzf_inflate).

        `members_bytes`: bytes / uint8 array; member k is members_bytes[member_off[k]:member_off[k + 1]].  Returns
        (text, dst_off, status): the inflated bytes as one uint8 array with member k's at text[dst_off[k]:dst_off[k + 1]],
        dst_off uint64 [n + 1] (the running sum of the ISIZE fields) and one BV_BGZF_* status per member; a member whose status is
        not BV_BGZF_OK leaves its range unspecified.  With `dst_ptr` (a device pointer of `dst_capacity` bytes) the bytes are
        written there instead and `text` is None."""
        data = np.frombuffer(members_bytes, dtype=np.uint8) if isinstance(members_bytes, (bytes, bytearray)) else np.ascontiguousarray(members_bytes, np.uint8)
        off = np.ascontiguousarray(member_off, dtype=np.uint64)
        n = int(off.size) - 1
        if n < 0:
            raise ValueError("bgzf_inflate: member_off needs n + 1 entries")
        mb = _capi.BgzfMembers(data.ctypes.data if data.size else None, off.ctypes.data, int(data.size), n, 0)
        dst_off = np.zeros(n + 1, dtype=np.uint64)
        status = np.zeros(n, dtype=np.uint8)
        args = (dst_off.ctypes.data, status.ctypes.data if n else None, None)
        if dst_ptr:
            text = None
            rc = self._lib.bv_engine_bgzf_inflate(self._h, C.byref(mb), int(dst_ptr), int(dst_capacity), _capi.BV_MEM_DEVICE, *args)
        else:
            # a call without room: the engine reads the ISIZE fields, writes dst_off and refuses; then the call with that room
            text = np.zeros(0, dtype=np.uint8)
            rc = self._lib.bv_engine_bgzf_inflate(self._h, C.byref(mb), None, 0, _capi.BV_MEM_HOST, *args)
            if rc == _capi.BV_ERR_INVALID_ARG and int(dst_off[n]) > 0:
                text = np.zeros(int(dst_off[n]), dtype=np.uint8)
                rc = self._lib.bv_engine_bgzf_inflate(self._h, C.byref(mb), text.ctypes.data, int(text.size), _capi.BV_MEM_HOST, *args)
        if rc != 0:
            raise RuntimeError("bv_engine_bgzf_inflate failed (%d): %s" % (rc, self._err()))
        return text, dst_off, status

    # ---- text, deflated into BGZF members on the device
    def bgzf_deflate(self, text, block_bytes=0xff00, block_off=None, level="fast"):
        """Text in, whole BGZF members out (bv_engine_bgzf_deflate_level): one member per block of `block_bytes` bytes (1 .. 0xff00;
        the last block takes what is left), or per block text[block_off[k]:block_off[k + 1]] where `block_off` is given.
        `level`: "fast" (the default: the fixed Huffman codes, about twice zlib level 6's size) or "small" (dynamic codes over
        16-, 8- and 4-byte grams: within 7 % of zlib level 6 for more kernel time, one workgroup per CU; README has the measured times).

        `text`: bytes / uint8 array, or a uint8 torch tensor on the engine's device, which is read where it lies (the caller has
        synchronised what wrote it).  Returns (members, member_off): the members back to back as one uint8 array, member k at
        members[member_off[k]:member_off[k + 1]], member_off uint64 [n + 1].  No end-of-file marker is appended."""
        keep = text
        if hasattr(text, "data_ptr"):  # a torch tensor
            if text.dtype.itemsize != 1 or not text.is_contiguous():
                raise ValueError("bgzf_deflate: a contiguous tensor of bytes")
            kind = _capi.BV_MEM_DEVICE if text.is_cuda else _capi.BV_MEM_HOST
            ptr, size = int(text.data_ptr()), int(text.numel())
        else:
            keep = np.frombuffer(text, dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, np.uint8)
            kind, ptr, size = _capi.BV_MEM_HOST, (keep.ctypes.data if keep.size else None), int(keep.size)
        return self._deflate("bgzf_deflate", "bv_engine_bgzf_deflate_level", size, block_bytes, block_off, level, (ptr, size, kind))  # (`keep` lives through it)

    def _deflate(self, who, symbol, size, block_bytes, block_off, level, text=()):
        """What bgzf_deflate, vcf_deflate and pileup_text_deflate share: the blocks of a text of `size` bytes, the level, room for
        the members, the call `symbol` (`text`: its arguments that name the text, if it takes any) and (members, member_off)."""
        if block_off is None:
            if not 1 <= int(block_bytes) <= 0xff00:
                raise ValueError("%s: block_bytes is 1 to 0xff00" % who)
            off = np.append(np.arange(0, size, int(block_bytes), dtype=np.uint64), np.uint64(size)) if size else np.zeros(1, np.uint64)
        else:
            off = np.ascontiguousarray(block_off, dtype=np.uint64)
        n = int(off.size) - 1
        if n < 0:
            raise ValueError("%s: block_off needs n + 1 entries" % who)
        if level not in _capi.DEFLATE_LEVELS:
            raise ValueError("%s: level is 'fast' or 'small'" % who)
        members = np.zeros(size + 31 * n, dtype=np.uint8)
        member_off = np.zeros(n + 1, dtype=np.uint64)
        rc = getattr(self._lib, symbol)(self._h, *text, off.ctypes.data, n, _capi.DEFLATE_LEVELS[level], members.ctypes.data if members.size else None,
                                        int(members.size), member_off.ctypes.data, None)
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (symbol, rc, self._err()), rc)
        return members[:int(member_off[n])], member_off

    def _text_fetch(self, symbol, size, dst_ptr, dst_capacity):
        """vcf_fetch and pileup_text_fetch: the `size` bytes of the text behind the call `symbol`, or its copy to `dst_ptr`"""
        if dst_ptr:
            rc = getattr(self._lib, symbol)(self._h, int(dst_ptr), int(dst_capacity), _capi.BV_MEM_DEVICE, None)
            text = None
        else:
            text = np.zeros(size, dtype=np.uint8)
            rc = getattr(self._lib, symbol)(self._h, text.ctypes.data if text.size else None, int(text.size), _capi.BV_MEM_HOST, None)
        if rc != 0:
            raise RuntimeError("%s failed (%d): %s" % (symbol, rc, self._err()), rc)
        return text

    # ---- VCF sample columns, written on the device (include/basevar_amd_vcf.h)
    def vcf_format(self, site, heads, gt, slab=None):
        """The VCF lines of rows `site` (bv_engine_vcf_format): line k is heads[k] (bytes: the record through "GT:AB:SO:BP"), one
        GT:AB:SO:BP column per sample of row site[k], and a line break.  `gt`: uint8 [n_lines][4], per line and base A, C, G, T
        the character b"0" (REF), b"." or b"1" .. b"4" (the ALT's number).  `slab`: a _capi.Slab in host or device memory whose
        base_strand and qual planes are read, or None for the rows kept by this engine's last lrt_text / lrt_bgzf, in record
        order.  The text stays on the device (vcf_fetch, vcf_deflate); returns line_off uint64 [n_lines + 1]."""
        site = np.ascontiguousarray(site, dtype=np.uint32)
        n = int(site.size)
        if len(heads) != n:
            raise ValueError("vcf_format: one head per line")
        head = np.frombuffer(b"".join(bytes(h) for h in heads), dtype=np.uint8)
        head_off = np.zeros(n + 1, dtype=np.uint64)
        head_off[1:] = np.cumsum([len(h) for h in heads])
        gt = np.ascontiguousarray(gt, dtype=np.uint8).reshape(n, 4)
        lines = _capi.VcfLines(C.pointer(slab) if slab is not None else None, site.ctypes.data, head.ctypes.data if head.size else None,
                               head_off.ctypes.data, gt.ctypes.data, n, 0)
        line_off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.bv_engine_vcf_format(self._h, C.byref(lines), line_off.ctypes.data, None)
        if rc != 0:
            raise RuntimeError("bv_engine_vcf_format failed (%d): %s" % (rc, self._err()), rc)
        self._vcf_bytes = int(line_off[n])
        return line_off

    def vcf_fetch(self, dst_ptr=0, dst_capacity=0):
        """The text of the last vcf_format (bv_engine_vcf_fetch) as a uint8 array; with `dst_ptr`, a device pointer of
        `dst_capacity` bytes, it is copied there instead and None is returned."""
        return self._text_fetch("bv_engine_vcf_fetch", getattr(self, "_vcf_bytes", 0), dst_ptr, dst_capacity)

    def vcf_deflate(self, block_bytes=0xff00, block_off=None, level="fast"):
        """bgzf_deflate of the last vcf_format's text, read where it lies on the device (bv_engine_vcf_deflate): (members,
        member_off) as bgzf_deflate returns them, byte for byte what it returns for the fetched text."""
        return self._deflate("vcf_deflate", "bv_engine_vcf_deflate", getattr(self, "_vcf_bytes", 0), block_bytes, block_off, level)

    # ---- whole VCF records and CVG rows from the records, written on the device (include/basevar_amd_record_text.h)
    @staticmethod
    def record_text_on_device(sites, groups=None):
        """Per record, whether every number its VCF head and CVG row print lies inside the device formatter's domains
        (bv_record_text_on_device): bool [n].  `sites`: SITE_DTYPE [n]; `groups`: GROUP_DTYPE [n][n_groups] or None."""
        lib = _capi.load()
        sites = np.ascontiguousarray(sites, dtype=_capi.SITE_DTYPE).reshape(-1)
        n = int(sites.size)
        g = None if groups is None else np.ascontiguousarray(groups, dtype=_capi.GROUP_DTYPE).reshape(n, -1)
        G = 0 if g is None else int(g.shape[1])
        out = np.zeros(n, dtype=bool)
        for k in range(n):
            out[k] = bool(lib.bv_record_text_on_device(sites[k:k + 1].ctypes.data, g[k].ctypes.data if G else None, G))
        return out

    def _record_lines(self, who, sites, groups, chrom, pos, ref_char, group_names, host_text, n):
        """The bv_record_lines both calls share, and what it points into (to be kept alive through the call).  `sites` /
        `groups`: numpy arrays, or (device pointer, n) / (device pointer, n_groups)."""
        keep = []
        def arr(a, dtype):
            a = np.ascontiguousarray(a, dtype=dtype)
            keep.append(a)
            return a
        def texts(items):  # offsets and bytes of per-line texts; None entries are empty
            if items is None:
                return None, None
            if len(items) != n:
                raise ValueError("%s: one text (or None) per line" % who)
            items = [b"" if t is None else bytes(t) for t in items]
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(t) for t in items])
            buf = np.frombuffer(b"".join(items) or b"\0", dtype=np.uint8)
            keep.extend([off, buf])
            return off.ctypes.data, buf.ctypes.data
        L = _capi.RecordLines()
        if isinstance(sites, tuple):
            L.records, L.mem_kind = int(sites[0]), _capi.BV_MEM_DEVICE
            L.groups = int(groups[0]) if groups is not None else None
            G = int(groups[1]) if groups is not None else 0
        else:
            s = arr(sites, _capi.SITE_DTYPE).reshape(-1)
            L.records, L.mem_kind = s.ctypes.data if n else None, _capi.BV_MEM_HOST
            G = 0
            if groups is not None:
                g = arr(groups, _capi.GROUP_DTYPE).reshape(n, -1)
                G = int(g.shape[1])
                L.groups = g.ctypes.data if g.size else None
        names = [bytes(x) for x in (group_names or ())]
        if len(names) != G:
            raise ValueError("%s: one name per group" % who)
        chrom = bytes(chrom)
        cbuf, nbuf = arr(np.frombuffer(chrom or b"\0", dtype=np.uint8), np.uint8), arr(np.frombuffer(b"".join(names) or b"\0", dtype=np.uint8), np.uint8)
        noff = np.zeros(G + 1, dtype=np.uint32)
        noff[1:] = np.cumsum([len(x) for x in names])
        keep.append(noff)
        p, r = arr(pos, np.uint32).reshape(-1), arr(np.frombuffer(bytes(ref_char), dtype=np.uint8) if isinstance(ref_char, (bytes, bytearray)) else ref_char, np.uint8).reshape(-1)
        if p.size != n or r.size != n:
            raise ValueError("%s: one pos and one ref_char per line" % who)
        L.pos, L.ref_char = (p.ctypes.data, r.ctypes.data) if n else (None, None)
        L.chrom, L.chrom_len = cbuf.ctypes.data, len(chrom)
        L.group_names, L.group_name_off = (nbuf.ctypes.data, noff.ctypes.data) if G else (None, None)
        L.host_text_off, L.host_text = texts(host_text)
        L.n_lines, L.n_groups, L.reserved_ = n, G, 0
        return L, keep, texts

    def cvg_format(self, sites, chrom, pos, ref_char, indel=None, host_text=None, groups=None, group_names=()):
        """The CVG rows of the records (bv_engine_cvg_format): row k from sites[k], `chrom`, pos[k], ref_char[k] and the row's
        indel column indel[k] (bytes; None or b"": "."), or host_text[k] where that is given (the whole row with its line break:
        the records bv_record_text_on_device refuses).  `sites`: SITE_DTYPE [n], or (device pointer, n).  The text stays on the
        device (cvg_fetch, cvg_deflate); returns line_off uint64 [n + 1]."""
        n = int(sites[1]) if isinstance(sites, tuple) else int(np.asarray(sites).size)
        L, keep, texts = self._record_lines("cvg_format", sites, groups, chrom, pos, ref_char, group_names, host_text, n)
        L.indel_off, L.indel = texts(indel)
        line_off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.bv_engine_cvg_format(self._h, C.byref(L), line_off.ctypes.data, None)
        if rc != 0:
            self._cvg_bytes = 0
            raise RuntimeError("bv_engine_cvg_format failed (%d): %s" % (rc, self._err()), rc)
        self._cvg_bytes = int(line_off[n])
        return line_off

    def cvg_fetch(self, dst_ptr=0, dst_capacity=0):
        """The text of the last cvg_format (bv_engine_cvg_fetch), as vcf_fetch returns vcf_format's."""
        return self._text_fetch("bv_engine_cvg_fetch", getattr(self, "_cvg_bytes", 0), dst_ptr, dst_capacity)

    def cvg_deflate(self, block_bytes=0xff00, block_off=None, level="fast"):
        """bgzf_deflate of the last cvg_format's text, read where it lies on the device (bv_engine_cvg_deflate)."""
        return self._deflate("cvg_deflate", "bv_engine_cvg_deflate", getattr(self, "_cvg_bytes", 0), block_bytes, block_off, level)

    # ---- the CVG rows' indel columns, tallied on the device (include/basevar_amd_indel.h)
    @staticmethod
    def indel_row_tokens_max():
        """The most tokens a row of indel_tally may have (bv_indel_row_tokens_max)."""
        return int(_capi.load().bv_indel_row_tokens_max())

    def indel_tally(self, key, tokens=None, text=None):
        """The indel columns of rows `key` (bv_engine_indel_tally): row k's tokens are those whose pos equals key[k].  `tokens`:
        a PILEUP_TOKEN_DTYPE array ascending by pos with `text` (bytes or uint8 array) in host memory; or (device pointer,
        n_tokens) with `text` = (device pointer, text_bytes); or None: the tokens of this engine's last pileup, where they lie.
        The columns stay on the device (indel_fetch, cvg_format_tallied); returns (col_off uint64 [n + 1], row_flag uint8 [n]:
        1 where the row is outside the tally's domain and its zero-length column is the caller's)."""
        key = np.ascontiguousarray(key, dtype=np.uint32).reshape(-1)
        n = int(key.size)
        T = None
        if tokens is not None:
            T = _capi.IndelTokens()
            if isinstance(tokens, tuple):
                T.tokens, T.n_tokens, T.mem_kind = int(tokens[0]) or None, int(tokens[1]), _capi.BV_MEM_DEVICE
                T.text, T.text_bytes = int(text[0]) or None, int(text[1])
            else:
                tk = np.ascontiguousarray(tokens, dtype=_capi.PILEUP_TOKEN_DTYPE).reshape(-1)
                tx = np.frombuffer(bytes(text), dtype=np.uint8) if isinstance(text, (bytes, bytearray)) else np.ascontiguousarray(text, dtype=np.uint8).reshape(-1)
                T.tokens, T.n_tokens, T.mem_kind = tk.ctypes.data if tk.size else None, int(tk.size), _capi.BV_MEM_HOST
                T.text, T.text_bytes = tx.ctypes.data if tx.size else None, int(tx.size)
            T.reserved_ = 0
        col_off = np.zeros(n + 1, dtype=np.uint64)
        row_flag = np.zeros(n, dtype=np.uint8)
        rc = self._lib.bv_engine_indel_tally(self._h, C.byref(T) if T is not None else None, key.ctypes.data if n else None, n, col_off.ctypes.data,
                                             row_flag.ctypes.data if n else None, None)
        if rc != 0:
            raise RuntimeError("bv_engine_indel_tally failed (%d): %s" % (rc, self._err()), rc)
        self._indel_bytes = int(col_off[n])
        return col_off, row_flag

    def indel_fetch(self, dst_ptr=0, dst_capacity=0):
        """The columns of the last indel_tally back to back (bv_engine_indel_fetch), as vcf_fetch returns vcf_format's text."""
        return self._text_fetch("bv_engine_indel_fetch", getattr(self, "_indel_bytes", 0), dst_ptr, dst_capacity)

    def cvg_format_tallied(self, sites, chrom, pos, ref_char, host_text=None, groups=None, group_names=()):
        """cvg_format with row k's indel column taken from column k of the last indel_tally, where it lies
        (bv_engine_cvg_format_tallied).  A row the tally flagged brings its host text."""
        n = int(sites[1]) if isinstance(sites, tuple) else int(np.asarray(sites).size)
        L, keep, _ = self._record_lines("cvg_format_tallied", sites, groups, chrom, pos, ref_char, group_names, host_text, n)
        line_off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.bv_engine_cvg_format_tallied(self._h, C.byref(L), line_off.ctypes.data, None)
        if rc != 0:
            self._cvg_bytes = 0
            raise RuntimeError("bv_engine_cvg_format_tallied failed (%d): %s" % (rc, self._err()), rc)
        self._cvg_bytes = int(line_off[n])
        return line_off

    def vcf_format_records(self, site, sites, chrom, pos, ref_char, groups=None, group_names=(), host_text=None, slab=None):
        """Whole VCF lines from the records (bv_engine_vcf_format_records): line k is the head of sites[k] -- formatted on the
        device, or host_text[k] (CHROM through "GT:AB:SO:BP") where that is given -- and the sample columns of row site[k] as
        vcf_format writes them, the gt characters derived from ref_char[k] and the record's ALTs.  A record without ALT and
        without host text gives an empty line.  `sites`, `groups`: numpy arrays ([n], [n][n_groups]) or (device pointer, n) /
        (device pointer, n_groups); `slab` as vcf_format's.  The text is vcf_fetch's / vcf_deflate's; returns line_off [n + 1]."""
        site = np.ascontiguousarray(site, dtype=np.uint32)
        n = int(site.size)
        L, keep, _ = self._record_lines("vcf_format_records", sites, groups, chrom, pos, ref_char, group_names, host_text, n)
        L.site = site.ctypes.data if n else None
        if slab is not None:
            L.slab = C.pointer(slab)
        line_off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.bv_engine_vcf_format_records(self._h, C.byref(L), line_off.ctypes.data, None)
        if rc != 0:
            raise RuntimeError("bv_engine_vcf_format_records failed (%d): %s" % (rc, self._err()), rc)
        self._vcf_bytes = int(line_off[n])
        return line_off

    # ---- BAM records, piled up on the device (include/basevar_amd_pileup.h)
    def pileup_set_reference(self, seq):
        """The contig's bases (str / bytes / uint8 array, letter case kept) for pileup and pileup_rows (bv_engine_pileup_set_reference)."""
        if isinstance(seq, str):
            seq = seq.encode()
        buf = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, np.uint8)
        rc = self._lib.bv_engine_pileup_set_reference(self._h, buf.ctypes.data if buf.size else None, int(buf.size))
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_set_reference failed (%d): %s" % (rc, self._err()), rc)

    def pileup(self, records, run_off, run_sample, n_samples, tid, region, window, mapq_thd, pitch=None, reserved=0):
        """The samples' raw BAM records piled up into engine-owned planes (bv_engine_pileup); returns the number of covered rows.

        `records`: bytes / uint8 array (host), a uint8 torch tensor on the engine's device, or an int device pointer; run r is
        records[run_off[r]:run_off[r + 1]], whole records of sample run_sample[r] (non-decreasing), in file order.  `region`:
        (region_beg, region_end), from where the 500 kb steps are laid out; `window`: (beg, end), 1-based inclusive, inside one step.
        `pitch`: cells of a plane row, default n_samples rounded up to 16."""
        keep = records
        if isinstance(records, int):
            kind, ptr = _capi.BV_MEM_DEVICE, records
        elif hasattr(records, "data_ptr"):
            if records.dtype.itemsize != 1 or not records.is_contiguous():
                raise ValueError("pileup: a contiguous tensor of bytes")
            kind, ptr = (_capi.BV_MEM_DEVICE if records.is_cuda else _capi.BV_MEM_HOST), int(records.data_ptr())
        else:
            keep = np.frombuffer(records, dtype=np.uint8) if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, np.uint8)
            kind, ptr = _capi.BV_MEM_HOST, (keep.ctypes.data if keep.size else None)
        off = np.ascontiguousarray(run_off, dtype=np.uint64)
        samp = np.ascontiguousarray(run_sample, dtype=np.uint32)
        n_runs = int(samp.size)
        if n_runs and off.size != n_runs + 1:
            raise ValueError("pileup: run_off needs n_runs + 1 entries")
        pitch = (int(n_samples) + 15) // 16 * 16 if pitch is None else int(pitch)
        reads = _capi.PileupReads(ptr or None, off.ctypes.data if n_runs else None, samp.ctypes.data if n_runs else None, pitch, n_runs, int(n_samples),
                                  int(tid), int(region[0]), int(region[1]), int(window[0]), int(window[1]), int(mapq_thd), kind, int(reserved))
        n_cov = C.c_uint32(0)
        rc = self._lib.bv_engine_pileup(self._h, C.byref(reads), C.byref(n_cov), None)
        del keep
        if rc != 0:
            raise RuntimeError("bv_engine_pileup failed (%d): %s" % (rc, self._err()), rc)
        self._pileup_covered = int(n_cov.value)
        self._pileup_window_rows = int(window[1]) - int(window[0]) + 1
        return int(n_cov.value)

    def pileup_fetch(self):
        """The last pileup (bv_engine_pileup_fetch): dict of cell, qual, mapq uint8 [rows][pitch], rank uint16 [rows][pitch], depth
        uint32 [rows], tokens (_capi.PILEUP_TOKEN_DTYPE, sorted by (pos, sample)) and their text (uint8)."""
        res = _capi.PileupResult()
        res.mem_kind = _capi.BV_MEM_HOST
        rc = self._lib.bv_engine_pileup_fetch(self._h, C.byref(res), None)  # no buffers: the sizes
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_fetch failed (%d): %s" % (rc, self._err()), rc)
        rows, cells = int(res.rows), int(res.cells)
        out = dict(cell=np.zeros(cells, np.uint8), qual=np.zeros(cells, np.uint8), mapq=np.zeros(cells, np.uint8), rank=np.zeros(cells, np.uint16),
                   depth=np.zeros(rows, np.uint32), tokens=np.zeros(int(res.n_tokens), _capi.PILEUP_TOKEN_DTYPE), text=np.zeros(int(res.text_bytes), np.uint8))
        for k, v in out.items():
            setattr(res, k, v.ctypes.data if v.size else None)
        res.cells_capacity, res.rows_capacity, res.tokens_capacity, res.text_capacity = cells, rows, int(res.n_tokens), int(res.text_bytes)
        rc = self._lib.bv_engine_pileup_fetch(self._h, C.byref(res), None)
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_fetch failed (%d): %s" % (rc, self._err()), rc)
        pitch = cells // rows
        for k in ("cell", "qual", "mapq", "rank"):
            out[k] = out[k].reshape(rows, pitch)
        return out

    def pileup_rows(self, tagged=False):
        """The covered rows of the last pileup as a device slab (bv_engine_pileup_rows): (_capi.Slab ready for bv_engine_submit and
        valid until the next pileup, positions uint32 [n], depths uint32 [n])."""
        n = getattr(self, "_pileup_covered", 0)
        slab = _capi.Slab()
        pos, depth = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        rc = self._lib.bv_engine_pileup_rows(self._h, 1 if tagged else 0, C.byref(slab), pos.ctypes.data if n else None, depth.ctypes.data if n else None)
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_rows failed (%d): %s" % (rc, self._err()), rc)
        return slab, pos, depth

    def pileup_bgzf(self, members_bytes, member_off, runs, n_samples, tid, region, window, mapq_thd, pitch=None, reserved=0):
        """pileup() from BGZF members that are still compressed (bv_engine_pileup_bgzf); returns the number of covered rows.

        Member k is members_bytes[member_off[k]:member_off[k + 1]] (host: bytes / uint8 array), as bgzf_inflate takes them.
        `runs`: an array of _capi.PILEUP_BGZF_RUN_DTYPE, or rows of (sample, first_member, n_members, begin, end): run r is cut
        from the text of its members, from `begin` bytes into the first to `end` bytes of the last.  The rest as in pileup()."""
        buf = np.frombuffer(members_bytes, dtype=np.uint8) if isinstance(members_bytes, (bytes, bytearray)) else np.ascontiguousarray(members_bytes, np.uint8)
        off = np.ascontiguousarray(member_off, dtype=np.uint64)
        if isinstance(runs, np.ndarray) and runs.dtype == _capi.PILEUP_BGZF_RUN_DTYPE:
            rr = np.ascontiguousarray(runs)
        else:
            rows = np.asarray(runs, dtype=np.uint32).reshape(-1, 5)
            rr = np.zeros(len(rows), _capi.PILEUP_BGZF_RUN_DTYPE)
            for k, f in enumerate(("sample", "first_member", "n_members", "begin", "end")):
                rr[f] = rows[:, k]
        n_members = max(int(off.size) - 1, 0)
        pitch = (int(n_samples) + 15) // 16 * 16 if pitch is None else int(pitch)
        arg = _capi.PileupBgzf()
        arg.members = _capi.BgzfMembers(buf.ctypes.data if buf.size else None, off.ctypes.data if off.size else None, int(buf.size), n_members, 0)
        arg.runs = rr.ctypes.data if rr.size else None
        arg.pitch, arg.n_runs, arg.n_samples, arg.tid = pitch, int(rr.size), int(n_samples), int(tid)
        arg.region_beg, arg.region_end, arg.beg, arg.end = int(region[0]), int(region[1]), int(window[0]), int(window[1])
        arg.mapq_thd, arg.reserved_ = int(mapq_thd), int(reserved)
        n_cov = C.c_uint32(0)
        rc = self._lib.bv_engine_pileup_bgzf(self._h, C.byref(arg), C.byref(n_cov), None)
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_bgzf failed (%d): %s" % (rc, self._err()), rc)
        self._pileup_covered = int(n_cov.value)
        self._pileup_window_rows = int(window[1]) - int(window[0]) + 1
        return int(n_cov.value)

    def lrt_pileup_bgzf(self, members_bytes, member_off, runs, n_samples, tid, region, window, mapq_thd, pitch=None, tagged=False):
        """lrt_pileup from compressed members: pileup_bgzf, pileup_rows and bv_engine_submit of the device slab; a PileupBatch."""
        self.pileup_bgzf(members_bytes, member_off, runs, n_samples, tid, region, window, mapq_thd, pitch=pitch)
        return self._lrt_piled(tagged)

    def lrt_pileup(self, records, run_off, run_sample, n_samples, tid, region, window, mapq_thd, pitch=None, tagged=False):
        """Reads in, records out: pileup, pileup_rows and bv_engine_submit of the device slab.  Returns a PileupBatch: the records
        of the covered rows, their positions and depths, and the indel tokens {(pos, sample): text}."""
        self.pileup(records, run_off, run_sample, n_samples, tid, region, window, mapq_thd, pitch=pitch)
        return self._lrt_piled(tagged)

    def _lrt_piled(self, tagged):
        """the engine's pileup through pileup_rows and bv_engine_submit"""
        slab, pos, depth = self.pileup_rows(tagged=tagged)
        res = _capi.PileupResult()
        res.mem_kind = _capi.BV_MEM_HOST
        self._lib.bv_engine_pileup_fetch(self._h, C.byref(res), None)
        tokens, text = np.zeros(int(res.n_tokens), _capi.PILEUP_TOKEN_DTYPE), np.zeros(int(res.text_bytes), np.uint8)
        res.tokens, res.text = (tokens.ctypes.data if tokens.size else None), (text.ctypes.data if text.size else None)
        res.tokens_capacity, res.text_capacity = int(tokens.size), int(text.size)
        rc = self._lib.bv_engine_pileup_fetch(self._h, C.byref(res), None)
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_fetch failed (%d): %s" % (rc, self._err()), rc)
        n = int(slab.n_sites)
        out = np.zeros(n, dtype=_capi.SITE_DTYPE)
        if n:
            import torch  # the records of a device slab are device memory: a tensor holds them
            d_out = torch.zeros(n * _capi.SITE_DTYPE.itemsize, dtype=torch.uint8, device="cuda:%d" % self.device)
            torch.cuda.synchronize(self.device)
            if self._lib.bv_engine_submit(self._h, C.byref(slab), int(d_out.data_ptr()), None, None) != 0:
                raise RuntimeError("bv_engine_submit failed: %s" % self._err())
            self.wait()
            out = d_out.cpu().numpy().view(_capi.SITE_DTYPE).copy()
        ms1, ms2 = self.kernel_ms() if n else (0.0, 0.0)
        toks = {(int(t["pos"]), int(t["sample"])): text[int(t["text_off"]):int(t["text_off"]) + int(t["text_len"])].tobytes() for t in tokens}
        return PileupBatch(out, None, self.last_variant_count() if n else 0, ms1, ms2, pos, depth, toks)

    # ---- batchfile rows, written on the device from piled-up planes (include/basevar_amd_pileup_text.h)
    def _pileup_text_request(self, who, chrom, first, n, tile):
        """(bv_pileup_text, n rows, what it points to) of pileup_text's arguments"""
        chrom = chrom.encode() if isinstance(chrom, str) else bytes(chrom)
        keep, t = [], None
        if tile is not None:
            planes = [tile[k] for k in ("cell", "qual", "mapq", "rank")]
            on_device = hasattr(planes[0], "data_ptr")
            if on_device:
                if any(not p.is_cuda or not p.is_contiguous() for p in planes):
                    raise ValueError(who + ": contiguous planes, all on the device or all numpy arrays")
                rows, pitch = int(planes[0].shape[0]), int(planes[0].shape[1])
                ptrs = [int(p.data_ptr()) for p in planes]
            else:
                planes = [np.ascontiguousarray(p, np.uint16 if i == 3 else np.uint8) for i, p in enumerate(planes)]
                rows, pitch = planes[0].shape
                ptrs = [p.ctypes.data for p in planes]
            tok = np.ascontiguousarray(tile.get("tokens", np.zeros(0, _capi.PILEUP_TOKEN_DTYPE)), _capi.PILEUP_TOKEN_DTYPE)
            text = np.ascontiguousarray(tile.get("text", np.zeros(0, np.uint8)), np.uint8)
            t = _capi.PileupTile(ptrs[0], ptrs[1], ptrs[2], ptrs[3], tok.ctypes.data if tok.size else None, text.ctypes.data if text.size else None,
                                 int(tile.get("pitch", pitch)), int(tok.size), int(text.size), int(tile["beg"]), int(tile.get("rows", rows)), int(tile["n_samples"]),
                                 int(tile.get("mem_kind", _capi.BV_MEM_DEVICE if on_device else _capi.BV_MEM_HOST)))
            keep = [planes, tok, text, t]
            total = int(t.rows)
        else:
            total = getattr(self, "_pileup_window_rows", 0)
        n = max(total - int(first), 0) if n is None else int(n)
        return _capi.PileupText(C.pointer(t) if t is not None else None, chrom, len(chrom), int(first), n, 0), n, keep

    def pileup_text(self, chrom, first=0, n=None, tile=None):
        """The batchfile rows of rows [first, first + n) of a tile (bv_engine_pileup_text): CHROM, pos, REF, Depth and the five
        lists of mapq, base, quality, rank and strand tokens, as host/pileup.hpp's pileup_rows_text writes them.  `tile` None: the
        last pileup where it lies on the device (n None: all its rows from `first`).  Else a dict: cell, qual, mapq (uint8) and
        rank (uint16) planes [rows][pitch] as numpy arrays (host) or torch tensors on the engine's device, beg, n_samples, tokens
        (_capi.PILEUP_TOKEN_DTYPE, ascending by (pos, sample)) and text (uint8, the tokens' text).  The text stays on the device
        (pileup_text_fetch, pileup_text_deflate); returns row_off uint64 [n + 1]."""
        req, n, keep = self._pileup_text_request("pileup_text", chrom, first, n, tile)
        row_off = np.zeros(n + 1, dtype=np.uint64)
        rc = self._lib.bv_engine_pileup_text(self._h, C.byref(req), row_off.ctypes.data, None)
        del keep
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_text failed (%d): %s" % (rc, self._err()), rc)
        self._ptext_bytes = int(row_off[n])
        return row_off

    def pileup_text_parts(self, chrom, part_first, first=0, n=None, tile=None):
        """pileup_text over sample parts of the tile (bv_engine_pileup_text_parts): part p is the samples [part_first[p],
        part_first[p + 1]), and its rows are those of a tile that holds only these columns -- the Depth and the five lists are
        the part's.  The text is part-major: part 0's n rows, then part 1's, ...; returns row_off uint64 [n_parts * n + 1], row k
        of part p at index p * n + k.  pileup_text_fetch and pileup_text_deflate serve this text as they serve pileup_text's."""
        req, n, keep = self._pileup_text_request("pileup_text_parts", chrom, first, n, tile)
        pf = np.ascontiguousarray(part_first, dtype=np.uint32)
        n_parts = max(int(pf.size) - 1, 0)
        arg = _capi.PileupTextParts(C.pointer(req), pf.ctypes.data if pf.size else None, n_parts, 0)
        row_off = np.zeros(n_parts * n + 1, dtype=np.uint64)
        rc = self._lib.bv_engine_pileup_text_parts(self._h, C.byref(arg), row_off.ctypes.data, None)
        del keep
        if rc != 0:
            raise RuntimeError("bv_engine_pileup_text_parts failed (%d): %s" % (rc, self._err()), rc)
        self._ptext_bytes = int(row_off[n_parts * n])
        return row_off

    def pileup_text_fetch(self, dst_ptr=0, dst_capacity=0):
        """The text of the last pileup_text (bv_engine_pileup_text_fetch) as a uint8 array; with `dst_ptr`, a device pointer of
        `dst_capacity` bytes, it is copied there instead and None is returned."""
        return self._text_fetch("bv_engine_pileup_text_fetch", getattr(self, "_ptext_bytes", 0), dst_ptr, dst_capacity)

    def pileup_text_deflate(self, block_bytes=0xff00, block_off=None, level="fast"):
        """bgzf_deflate of the last pileup_text's text, read where it lies on the device (bv_engine_pileup_text_deflate): (members,
        member_off) as bgzf_deflate returns them, byte for byte what it returns for the fetched text."""
        return self._deflate("pileup_text_deflate", "bv_engine_pileup_text_deflate", getattr(self, "_ptext_bytes", 0), block_bytes, block_off, level)

    def deflate_code_lengths(self, counts, limit):
        """The code lengths the small deflate level gives an alphabet with these counts (bv_engine_deflate_code_lengths, a
        diagnostic): (lengths uint8 [n], rounds of halving)."""
        counts = np.ascontiguousarray(counts, dtype=np.uint32)
        lengths = np.zeros(counts.size, np.uint8)
        rounds = C.c_uint32(0)
        rc = self._lib.bv_engine_deflate_code_lengths(self._h, counts.ctypes.data, int(counts.size), int(limit), lengths.ctypes.data, C.byref(rounds), None)
        if rc != 0:
            raise RuntimeError("bv_engine_deflate_code_lengths failed (%d): %s" % (rc, self._err()), rc)
        return lengths, int(rounds.value)


class PileupBatch(BaseTypeBatch):
    """Records of BaseTypeEngine.lrt_pileup: one per covered row of the window, with the rows' 1-based positions and depths and
    the window's indel tokens {(pos, sample): text}."""

    def __init__(self, sites, groups, n_variant, pass1_ms, pass2_ms, positions, depth, tokens):
        BaseTypeBatch.__init__(self, sites, groups, n_variant, pass1_ms, pass2_ms)
        self.positions = positions
        self.depth = depth
        self.tokens = tokens


class TextBatch(BaseTypeBatch):
    """Records of BaseTypeEngine.lrt_text, plus the positions they belong to, the row states and the returned planes."""

    def __init__(self, sites, groups, n_variant, positions, row_state, cell, phred):
        super().__init__(sites, groups, n_variant, 0.0, 0.0)
        self.positions = positions
        self.row_state = row_state
        self.cell = cell
        self.phred = phred


def tile_packed_layout(n_sites, width, with_ranks=True, with_groups=False):
    """(pitch, [offsets of base_strand, qual, mapq, rpr, group_id], total bytes) of a packed host tile: one allocation
    that bv_engine_tiles_add sends over the link as one copy (include/basevar_amd.h)."""
    lib = _capi.load()
    pitch, total = C.c_uint64(), C.c_uint64()
    offs = (C.c_uint64 * 5)()
    rc = lib.bv_tile_packed_layout(n_sites, width, 1 if with_ranks else 0, 1 if with_groups else 0, C.byref(pitch), offs,
                                   C.byref(total))
    if rc != 0:
        raise RuntimeError("bv_tile_packed_layout failed (%d)" % rc)
    return pitch.value, [int(o) for o in offs], total.value


def synth_fill(device, n_sites, n_samples, pitch, base_strand, qual, ref_base, mapq=0, rpr=0, seed=0xBA5E7A7,
               site_offset=0, coverage=0.08, indel_frac=0.005, qual_mean=32.0, qual_sd=6.0, qual_min=2, qual_max=41,
               stream=0, layout=0):
    """Device-side synthetic pileup (bench helper): all pointers are device pointers (ints)."""
    lib = _capi.load()
    sp = _capi.SynthParams(int(seed), int(site_offset), float(coverage), float(indel_frac), float(qual_mean),
                           float(qual_sd), int(qual_min), int(qual_max), int(layout))
    rc = lib.bv_synth_fill(int(device), C.byref(sp), int(n_sites), int(n_samples), int(pitch), base_strand, qual,
                           mapq or None, rpr or None, ref_base, stream or None)
    if rc != 0:
        raise RuntimeError("bv_synth_fill failed (%d): %s" % (rc, lib.bv_last_error(None).decode()))
