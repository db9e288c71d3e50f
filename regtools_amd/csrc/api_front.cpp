// api_front.cpp -- the front of one call (EventsRun, api_internal.h): the file on its way to HBM, the BGZF member list, the DEFLATE launch.
#include "api_internal.h"

int EventsRun::run() {
    if (!p || p->strandness < 0 || p->strandness > 3) return fail(err, errlen, RGX_ERR_ARG, "Please supply strandness mode with '-s' option!\n\n");
    if (p->strandness == 3 && !p->fasta_path) return fail(err, errlen, RGX_ERR_ARG, "Strandness mode 'intron-motif' requires a fasta file!\n\n");
    HIP_ENTER(c->device);
    st = c->stream;
    copy_q = c->copy_stream ? c->copy_stream : c->stream;     // where the file's upload goes (a one-shot context: its only stream)
    t_begin = now_ms();
    trace = getenv("REGTOOLS_AMD_TRACE") != nullptr;
    t_last = t_begin;

    if (bam_len < 28) return fail(err, errlen, RGX_ERR_OPEN, "%s", kMsgOpen);
    // (the arena the last call's data lay in, after it lost its place)
    if (c->arena_retired) { c->arena_retired->release(); delete c->arena_retired; c->arena_retired = nullptr; }
    // (anything but kGoOn: an error, or kRestart -- prepare_events builds the next attempt)
    { const int rc = stage_upload(); if (rc != kGoOn) return rc; }
    { const int rc = stage_members(); if (rc != kGoOn) return rc; }
    { const int rc = stage_range_and_inflate(); if (rc != kGoOn) return rc; }
    { const int rc = stage_footers_and_header(); if (rc != kGoOn) return rc; }
    { const int rc = stage_bounds_and_chains(); if (rc != kGoOn) return rc; }
    { const int rc = stage_framing(); if (rc != kGoOn) return rc; }
    { const int rc = stage_decode(); if (rc != kGoOn) return rc; }
    const int rc_emit = stage_emit();
    if (rc_emit == RGX_OK) { const int rc = calibrate_arena(); if (rc != RGX_OK) return rc; }
    P.d_file = rc_emit == RGX_OK && p->n_shards <= 1 && region_kind(p->region) == RegionKind::whole ? d_bam : nullptr;      // (every byte of the file went up)
    return rc_emit;
}

// Arena placement trials (rgx_ctx above) -- OPT-IN (REGTOOLS_AMD_ARENA=5) since round 6.  On a context's first call with an arena of 2 GiB and more
// (and again when a later one is a quarter larger), once the call's own work is enqueued: the same whole-range launch, plain, into the call's arena and into
// fresh allocations ONE AT A TIME (a warm-up launch, then the median of three timed with HIP events); a challenger that beats the incumbent's median by 1.5 %
// becomes the context's arena (rgx_ctx_arena_trials reports the times).  The call's data stays where it is -- when a challenger wins, the old arena is
// retired and released by the next call.  At most ONE arena's worth of extra memory is ever held, free memory is asked for again before every candidate, and
// anything that goes wrong inside a trial leaves the incumbent in place: the caller's result is complete before the first trial starts.
static int arena_challengers() { return arena_knobs().trials; }
int EventsRun::calibrate_arena() {
    if (!arena_challengers() || c->one_shot || d_true_sizes || chunked || split_B || P.stream_ended || !n_range || n_range <= 2048 ||
        total < ((uint64_t)2 << 30)) return RGX_OK;
    if (c->arena_calibrated_bytes == UINT64_MAX || (c->arena_calibrated_bytes &&
        total + 256 <= c->arena_calibrated_bytes + c->arena_calibrated_bytes / 4)) return RGX_OK;
    // (one calibration at a time per DEVICE: the arenas of different devices have nothing to do with one another)
    static std::mutex trial_mu[16];
    std::lock_guard<std::mutex> trial_lock(trial_mu[(unsigned)c->device % 16u]);
    if (!inflate_takes_coop(n_range) || h_sc->inflate.first_bad != 0xffffffffu) return RGX_OK;
    DevBuf &b_arena = c->buf(Buf::arena), &b_lens = c->buf(Buf::inflate_scratch);
    if (!b_arena.p || b_arena.cap < total + 256) return RGX_OK;
    auto room_for_one = [&] {                                  // (a challenger AND what the call -- or a co-tenant of the device -- may still allocate)
        size_t free_b = 0, total_b = 0;
        return hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b >= b_arena.cap + b_arena.cap / 8 + ((size_t)16 << 30);
    };
    const int plan = inflate_plan_for(bam_len, total_all);
    uint32_t *d_dummy = &d_sc->trial_inflate.first_bad;         // (the trial launches' verdicts: not looked at -- the call's own launch gave the verdict)
    auto time_into = [&](uint8_t *arena_p, float &ms) -> hipError_t {
        float t[3] = {0, 0, 0};
        for (int k = 0; k < 4; ++k) {                          // (the first launch into a fresh allocation also pays for its pages: not timed)
            hipError_t e = hipMemsetAsync(d_dummy, 0xff, sizeof d_sc->trial_inflate, st);
            if (e != hipSuccess) return e;
            if ((e = hipEventRecord(c->ev_trial[0], st)) != hipSuccess) return e;
            launch_inflate(d_bam, d_members + m_lo, n_range, arena_p, upos_lo, b_lens.as<uint32_t>(), d_dummy, st, 0, 0, false, 0, nullptr, plan);
            if ((e = hipEventRecord(c->ev_trial[1], st)) != hipSuccess) return e;
            if ((e = hipEventSynchronize(c->ev_trial[1])) != hipSuccess) return e;
            if (k && (e = hipEventElapsedTime(&t[k - 1], c->ev_trial[0], c->ev_trial[1])) != hipSuccess) return e;
        }
        std::sort(t, t + 3);
        ms = t[1];
        return hipSuccess;
    };
    c->arena_trials = 0;
    float best_ms = 0;
    // (the call's own arena: the same bytes written once more, behind everything that read them)
    if (time_into(b_arena.as<uint8_t>(), best_ms) != hipSuccess) { (void)hipGetLastError(); return RGX_OK; }
    c->arena_trial_ms[c->arena_trials++] = best_ms;
    DevBuf best;                                               // the fastest challenger so far (empty: the incumbent leads)
    for (int k = 0; k < arena_challengers(); ++k) {
        if (best.p) break;                                     // (a winner is kept at once: never two challengers' memory at a time)
        if (!room_for_one()) break;
        // (what makes one placement faster than another is not known -- DESIGN 5.5 -- so the challengers are not of one kind)
        // (a hipMalloc block never won one: 15.6-16.3 ms beside 12.7-13.6)
        static const size_t kLadder[] = {(size_t)1 << 30, (size_t)256 << 20, (size_t)512 << 20, (size_t)128 << 20, (size_t)1 << 30, (size_t)64 << 20,
            (size_t)512 << 20};
        DevBuf cand; cand.piece = b_arena.piece ? kLadder[k % 7] : 0;
        if (cand.ensure(b_arena.cap) != hipSuccess) { (void)hipGetLastError(); break; }
        float ms = 0;
        if (time_into(cand.as<uint8_t>(), ms) != hipSuccess) { (void)hipGetLastError(); cand.release(); break; }
        if (c->arena_trials < 8) c->arena_trial_ms[c->arena_trials++] = ms;
        if (ms < best_ms * 0.985f) { best = std::move(cand); best_ms = ms; } else cand.release();
    }
    const bool challenger_kept = best.p != nullptr;
    if (challenger_kept) {
        // the call's data lies in the old arena and the caller may still read it (P.arena): it is retired, not released
        if (c->arena_retired) { c->arena_retired->release(); delete c->arena_retired; }
        c->arena_retired = new DevBuf(std::move(b_arena));
        b_arena = std::move(best);
        b_arena.piece = arena_knobs().piece;                   // (a later regrow is made of the configured pieces, not of the winner's ladder size)
    }
    c->arena_calibrated_bytes = b_arena.cap;
    if (trace) {
        fprintf(stderr, "[rgx trace] arena placement: call's arena %.3f ms", c->arena_trial_ms[0]);
        for (int k = 1; k < c->arena_trials; ++k) fprintf(stderr, ", %.3f", c->arena_trial_ms[k]);
        fprintf(stderr, " -> %s\n", challenger_kept ? "a challenger kept" : "kept");
    }
    mark("arena placement trial");
    return RGX_OK;
}

int EventsRun::stage_upload() {
    // -- upload ----------------------------------------------------------------------------------------------------------
    // Host input: the file goes up in chunks on the copy stream from a helper thread (a pageable source makes hipMemcpyAsync block), while
    // this thread finds the members on the host (scan_members_parallel) -- the inflate of chunk k's members then runs while chunk k+1 is
    // still on the bus (SURVEY 8d times the path from file bytes in host memory).  A file the host scan does not vouch for waits for the
    // whole upload and takes the device's member discovery, as does device input.
    d_bam = d_bam_in;
    hm.clear();
    if (!d_bam) {
        DevBuf &b = c->buf(Buf::bam);
        HIP_TRY(b.ensure(bam_len + 64));
        d_bam = b.as<uint8_t>();
        mark("file buffer in HBM");
        if (c->link) { c->wire_hold.take(&c->link->wire); mark("the link is ours"); }
        const size_t overlap_min = overlap_knobs().min_bytes;
        if (!d_true_sizes && bam_len >= overlap_min) {
            HIP_TRY(ensure_upload_streams(c));
            if (c->copy_stream) copy_q = c->copy_stream;
            mark("upload streams");
            // A shard of a file whose members the caller scanned: only the bytes this shard reads go up -- the header's members and the
            // range between its two cuts (stage_members' cuts: shard_cut_targets, from the index) -- N shards then move the file once, not N times.
            UploadRange ur{0, bam_len, 0};
            if (shared && p->n_shards > 1 && p->shard >= 0 && p->shard < p->n_shards) {
                ix.join();
                BamHeader hh; size_t hb = 0;
                if (ix.ok && host_bam_header(h_bam, std::min<size_t>(bam_len, (size_t)8 << 20), hh, &hb)) {
                    const RegionKind kind = region_kind(p->region);
                    uint64_t sv = 0;
                    if (kind == RegionKind::rest && bi.have_nocoor) sv = bi.nocoor_voff; else if (kind == RegionKind::whole && bi.have_start) sv = bi.start_voff;
                    uint64_t tgt[2], got[2];
                    shard_cut_targets(bam_len, p->shard, p->n_shards, sv ? sv : 1, tgt);
                    bai_first_anchor_ge(ix.bai, ix.bai_len, tgt, 2, got);
                    const std::vector<Member> &sm = *shared->members;
                    size_t m4_end = 0;
                    if (!sm.empty()) { const Member &m4 = sm[std::min<size_t>(sm.size(), 4) - 1]; m4_end = (size_t)m4.cpos + m4.clen + 8; }
                    ur = shard_upload_range(bam_len, p->shard, p->n_shards, got, hb, m4_end);
                }
            }
            const size_t up_lo = ur.lo, up_hi = ur.hi, hdr_hi = ur.hdr_hi;
            // Round 4: ONE inflate launch for the whole range, its waves gated by the arrival of their upload chunk (kernels.h InflateGate):
            // the file goes up in kGateChunks equal chunks, a 4-byte copy of this call's epoch into the chunk's flag word queued right behind each.
            // The members of the early chunks start ~0.6 ms into the upload; only those of the last chunk pay the lane-serial floor behind it
            // (round 3: three launches, each ~10 ms for a third of the members, the last one started when the last third had arrived).
            // A one-shot context, or one whose gate once gave an unclean verdict: round 3's pieces.
            const unsigned gate_chunks = overlap_knobs().chunks;
            gated = !c->gate_distrust && !c->one_shot && up_hi - up_lo >= std::min(overlap_min, (size_t)8 << 20) &&
                up_hi - up_lo >= 2 * 4096 * (size_t)gate_chunks;
            // ... for payloads whose inflate is of the upload's order, judged by the file's first members
            if (gated) gated = payload_takes_gate(h_bam, bam_len);
            // (ungated: three pieces, each its own launch on its own hardware queue -- two side streams + the pipeline's own)
            UploadChunks uc = plan_upload_chunks(up_lo, up_hi, gated, gate_chunks, c->one_shot);
            if (gated) {
                DevBuf &bg = c->buf(Buf::gate_flags);
                if (!bg.p) { HIP_TRY(bg.ensure(4 * 64)); HIP_TRY(hipMemset(bg.p, 0, 4 * 64)); c->gate_epoch = 0; }
                ++c->gate_epoch;
            }
            gate_chunk = uc.gate_chunk; up.end = std::move(uc.end);
            up.lo = up_lo; up.hi = up_hi; up.hdr_hi = hdr_hi;
            while (c->chunk_ev.size() < up.end.size()) { hipEvent_t e; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); c->chunk_ev.push_back(e); }
            uint8_t *dst = b.as<uint8_t>();
            uint32_t *gate_flags = gated ? c->buf(Buf::gate_flags).as<uint32_t>() : nullptr;
            const uint32_t gate_epoch = c->gate_epoch;
            hipStream_t gate_q = c->side[0] ? c->side[0] : copy_q;
            if (trace && (up_lo || up_hi < bam_len)) fprintf(stderr, "[rgx trace] shard %d of %d: bytes [%zu, %zu) of %zu go up behind the header's [0, %zu)\n",
                p->shard, p->n_shards, up_lo, up_hi, bam_len, hdr_hi);
            up.th = std::thread([this, dst, hdr_hi, up_lo, gate_q, gate_flags, gate_epoch] {
                if (hipSetDevice(c->device) != hipSuccess) { up.err = 1; up.recorded = (uint32_t)up.end.size(); return; }
                if (hdr_hi && hipMemcpyAsync(dst, h_bam, hdr_hi, hipMemcpyHostToDevice, copy_q) != hipSuccess) up.err = 1;
                size_t o = up_lo;
                for (size_t j = 0; j < up.end.size(); ++j) {
                    if ((up.end[j] > o && hipMemcpyAsync(dst + o, h_bam + o, up.end[j] - o, hipMemcpyHostToDevice, copy_q) != hipSuccess) ||
                        hipEventRecord(c->chunk_ev[j], copy_q) != hipSuccess) up.err = 1;
                    if (trace && j == 0) fprintf(stderr, "[rgx trace] first chunk enqueued         %8.3f ms after the call's entry\n", now_ms() - t_begin);
                    // (the flag's one-lane kernel goes to a side stream behind the chunk's event: on the copy stream itself it sat between two
                    //  copies, ~30 us of an idle bus per chunk)
                    if (gate_flags) {
                        if (gate_q != copy_q && hipStreamWaitEvent(gate_q, c->chunk_ev[j], 0) != hipSuccess) up.err = 1;
                        launch_gate_set(gate_flags + j, gate_epoch, gate_q);
                        // (a refused launch is only in THIS thread's hipGetLastError: unread, the flag would never be set and every gated wave
                        //  would wait out its time-out)
                        if (hipGetLastError() != hipSuccess) up.err = 1;
                    }
                    o = up.end[j];
                    up.recorded.store((uint32_t)j + 1, std::memory_order_release);
                }
                // the file is on the device: the next call's upload may start.  A host function behind the last copy, not a wait in this thread -- a thread
                // blocked in hipEventSynchronize kept the call's own launches from being enqueued until the upload was over (round 6: the gated launch
                // went out 8.8 ms late).
                if (c->link && hipLaunchHostFunc(copy_q, [](void *h) { ((TurnHold *)h)->give(); }, &c->wire_hold) != hipSuccess) { (void)hipGetLastError();
                    c->wire_hold.give(); }
            });
            if (shared) { hm = *shared->members; hm_total = shared->total_inflated; overlap = !hm.empty(); }
            else overlap = scan_members_parallel(h_bam, bam_len, (int)usable_threads(24), hm, hm_total);
            mark("host member scan");
            if (!overlap) {       // not a file the host vouches for: everything on the device, after the last chunk
                up.th.join();
                if (up.err) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: upload failed\n");
                if (up_lo || up_hi < bam_len) {                 // (only a range went up: the rest before the device looks at the file)
                    if (up_lo > hdr_hi) HIP_TRY(hipMemcpyAsync(dst + hdr_hi, h_bam + hdr_hi, up_lo - hdr_hi, hipMemcpyHostToDevice, copy_q));
                    if (up_hi < bam_len) HIP_TRY(hipMemcpyAsync(dst + up_hi, h_bam + up_hi, bam_len - up_hi, hipMemcpyHostToDevice, copy_q));
                    HIP_TRY(hipEventRecord(c->chunk_ev[up.end.size() - 1], copy_q));
                }
                HIP_TRY(hipStreamWaitEvent(st, c->chunk_ev[up.end.size() - 1], 0));
            }
        } else HIP_TRY(hipMemcpyAsync(b.p, h_bam, bam_len, hipMemcpyHostToDevice, st));
    }
    DevBuf &b_scalars = c->buf(Buf::scalars);
    HIP_TRY(b_scalars.ensure(sizeof(Scalars)));
    d_sc = b_scalars.as<Scalars>();
    h_sc = (Scalars *)c->pinned;
    HIP_TRY(hipMemsetAsync(d_sc, 0, sizeof(Scalars), st));
    HIP_TRY(hipMemsetAsync(&d_sc->inflate.first_bad, 0xff, 4, st));
    HIP_TRY(hipMemsetAsync(&d_sc->hdr_inflate.first_bad, 0xff, 4, st));
    HIP_TRY(hipMemsetAsync(&d_sc->stop, 0xff, 4, st));
    HIP_TRY(hipMemsetAsync(&d_sc->inflate_early.first_bad, 0xff, 4, st));

    return kGoOn;
}

int EventsRun::stage_members() {
    // -- BGZF member discovery on the device (replaces the serial BSIZE walk, bgzf.c:421-546) -------------------------------
    DevBuf &b_members = c->buf(Buf::members);
    if (overlap) {
        // the member list came from the host scan: what the discovery kernels would have left in HBM.  It goes there from page-locked host memory
        // by a kernel on the pipeline's stream, one coalesced pass (a copy would queue behind the file's chunks on the copy engine, measured 4 ms).
        // Read in place by the kernels instead -- the lane sort, then every lane of the gated launch its own 24 bytes at wave start, 169 k scattered
        // reads whose completions share the link's direction with the upload -- it made the chunk under the launch take 1.04 ms instead of 0.59.
        n_cand = (uint32_t)hm.size();
        const size_t need = ((size_t)n_cand + 1) * sizeof(Member);
        if (need > c->pinned_members_cap) {
            if (c->pinned_members) (void)hipHostFree(c->pinned_members);
            c->pinned_members = nullptr; c->pinned_members_cap = 0;
            HIP_TRY(hipHostMalloc(&c->pinned_members, need + need / 4, hipHostMallocDefault));
            c->pinned_members_cap = need + need / 4;
        }
        memcpy(c->pinned_members, hm.data(), (size_t)n_cand * sizeof(Member));
        HIP_TRY(b_members.ensure(need + 16));
        launch_members_fetch((const Member *)c->pinned_members, b_members.as<Member>(), n_cand, st);
        h_sc->n_members = n_cand; h_sc->total_inflated = hm_total;
        HIP_TRY(hipMemcpyAsync(&d_sc->n_members, &h_sc->n_members, 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(&d_sc->total_inflated, &h_sc->total_inflated, 8, hipMemcpyHostToDevice, st));
    } else {
        disc.c = c; disc.st = st; disc.d_bam = d_bam; disc.bam_len = bam_len; disc.d_true_sizes = d_true_sizes; disc.d_sc = d_sc; disc.h_sc = h_sc;
        { const int rc = disc.candidates(/*guarded=*/false, err, errlen); if (rc != kGoOn) return rc; }
        n_cand = disc.n_cand;
        if (n_cand == 0) return fail(err, errlen, RGX_ERR_OPEN, "%s", kMsgOpen);
    }
    d_members = b_members.as<Member>();
    h_members = overlap ? (const Member *)c->pinned_members : nullptr;
    from_members = overlap ? hipMemcpyHostToHost : hipMemcpyDeviceToHost;
    if (!overlap) disc.chain(UINT64_MAX);
    ix.join();
    if (!ix.ok) return (void)hipStreamSynchronize(st), fail(err, errlen, RGX_ERR_INDEX, "%s", kMsgIndex);
    mark("parse_bai");
    // (whole and rest both read to the end of the file without a predicate)
    const bool rest = region_kind(p->region) == RegionKind::rest;
    whole = region_kind(p->region) != RegionKind::query;
    // where the record stream starts (hts.c:1721-1741)
    if (rest) {
        if (bi.have_nocoor) { seek_voff = bi.nocoor_voff; seek = seek_voff != 0; }
        else if (!bi.n_no_coor) return (void)hipStreamSynchronize(st), fail(err, errlen, RGX_ERR_REGION, "%s", kMsgRegion);
    } else if (whole) {
        if (bi.have_start) { seek_voff = bi.start_voff; seek = seek_voff != 0; }
        else if (!bi.n_no_coor) return (void)hipStreamSynchronize(st), fail(err, errlen, RGX_ERR_REGION, "%s", kMsgRegion);
    }
    // shard cut points: virtual offsets the BAI lists (every chunk begin / linear-index entry is a record start), so
    // no shard ever guesses its first record.  A record belongs to the shard in which its first byte lies.
    cut_lo = seek ? seek_voff : 0; cut_hi = UINT64_MAX;          // 0 = "right after the header"
    if (p->n_shards > 1) {
        if (p->shard < 0 || p->shard >= p->n_shards) return (void)hipStreamSynchronize(st), fail(err, errlen, RGX_ERR_ARG, "regtools_amd: shard %d of %d\n",
            p->shard, p->n_shards);
        uint64_t tgt[2], got[2];
        shard_cut_targets(bam_len, p->shard, p->n_shards, seek ? seek_voff : 1, tgt);
        bai_first_anchor_ge(ix.bai, ix.bai_len, tgt, 2, got);
        if (p->shard > 0) cut_lo = got[0];
        if (p->shard + 1 < p->n_shards) cut_hi = got[1];
        if (cut_hi < cut_lo) cut_hi = cut_lo;
        mark("shard cuts");
    }

    // region queries: the reference's iterator reads the CHUNKS the index lists for the region's bins, one seek each, and ends at the first
    // record it reads that lies on another contig or at / behind the region's end (hts_itr_query / hts_itr_next, hts.c:1733-1800, :1924-1965).
    // The chunk list is computed here, from the index; the members between the first chunk's begin and the last one's end are inflated,
    // every chunk becomes its own record chain (SegGeom) and k_decode_seg applies the end rule.  Needs the contig names before the
    // launch: the header is inflated on the host from the head of the file.  A header that cannot be read that way leaves the range
    // alone: the whole file is read and filtered by overlap (such a header is not readable upstream either).
    geom_chunked_hint = !whole;                    // (region queries keep the checked path: their chunk table wants the members' verdicts)
    if (!whole && p->region) {
        const size_t head_len = std::min<size_t>(bam_len, (size_t)8 << 20);
        std::vector<uint8_t> head_copy;
        const uint8_t *head = h_bam;
        if (!head) { head_copy.resize(head_len); HIP_TRY(hipMemcpy(head_copy.data(), d_bam, head_len, hipMemcpyDeviceToHost)); head = head_copy.data(); }
        BamHeader hh;
        int32_t tid = -1, beg = 0, end = 0;
        // (the one parse of a call that talks: what sam_itr_querys -> hts_parse_decimal says about the region's numbers, once per query)
        if (host_bam_header(head, head_len, hh) && parse_region(hh, p->region, tid, beg, end,
            /*say=*/p->n_shards <= 1 || p->shard == 0) && tid < bi.n_ref && end >= beg &&
            region_chunks(ix.bai, ix.bai_len, tid, beg, end, chunks)) {
            chunked = true;
            if (p->n_shards > 1) {
                // a region query over several shards: the iterator's chunk list is dealt out in order, in runs of about equal compressed size;
                // shard g follows its run as an iterator of its own, and the one that meets the record that ends the iteration says so
                // (stream_ended): the merge ignores the shards behind it, as it does behind damage
                std::vector<uint64_t> before(chunks.size() + 1, 0);
                for (size_t k = 0; k < chunks.size(); ++k) before[k + 1] = before[k] + std::max<uint64_t>(1, (chunks[k].v >> 16) - (chunks[k].u >> 16));
                const uint64_t W = std::max<uint64_t>(1, before[chunks.size()]);
                std::vector<VChunk> mine;
                for (size_t k = 0; k < chunks.size(); ++k)
                    if ((int)std::min<uint64_t>((uint64_t)p->n_shards - 1, before[k] * (uint64_t)p->n_shards / W) == p->shard) mine.push_back(chunks[k]);
                chunks.swap(mine);
                cut_lo = seek ? seek_voff : 0; cut_hi = UINT64_MAX;     // (the byte cuts above were for a whole-file read)
            }
            if (!chunks.empty()) {
                // like the iterator's bgzf_seek: reading starts at the first chunk whatever the state of the members in front of it
                uint64_t hi = 0;
                for (const VChunk &ch : chunks) hi = std::max(hi, ch.v);
                cut_lo = chunks.front().u; cut_hi = std::max(hi, cut_lo); seek = true; seek_voff = cut_lo;
            // no bin of the region holds a record: nothing to inflate
            } else if (bi.have_start && bi.start_voff) { cut_lo = cut_hi = bi.start_voff; seek = true; seek_voff = cut_lo; }
        }
        mark("region chunks");
    }

    auto query = [&]() -> hipError_t {
        uint64_t q[3] = {seek ? (seek_voff >> 16) : 0, cut_lo >> 16, cut_hi == UINT64_MAX ? UINT64_MAX - 64 : (cut_hi >> 16)};
        if (overlap) {
            // the member list is on the host (scan_members_parallel): what k_member_query / k_member_stop would answer, without a round trip
            const uint32_t nm = (uint32_t)hm.size();
            const MemberQuery mq = host_member_query(hm.data(), nm, q);
            memcpy(h_sc->q_index, mq.q_index, sizeof mq.q_index); memcpy(h_sc->q_upos, mq.q_upos, sizeof mq.q_upos);
            h_sc->stop = mq.stop; h_sc->n_members = nm; h_sc->total_inflated = hm_total;
            return hipSuccess;
        }
        return disc.query(q);
    };
    HIP_TRY(query());
    if (seek && (seek_voff >> 16) != 0 && h_sc->q_index[0] >= h_sc->n_members) {
        // the host scan's list: the index points at something that is no member of this (well-formed) file -- the device's discovery decides what that means
        if (overlap) { mark("index points at no member: starting over device-resident"); return restart(Restart::index_points_at_no_member); }
        // the seek target is no member of the chain from offset 0: something in front of it is broken.  bgzf_seek (hts_itr_next, hts.c:1935)
        // goes there regardless -- take it as a second chain root.  (Only damaged files get here.)
        disc.chain(seek_voff >> 16);
        HIP_TRY(query());
        mark("second chain root");
        if (h_sc->q_index[0] >= h_sc->n_members) {
            // there is no BGZF member at the seek target at all (a truncated file, an index that belongs to another file): the
            // reference's read after bgzf_seek fails and the iterator returns nothing.  Keep the head of the file for the header only.
            disc.chain(UINT64_MAX);
            seek = false; cut_lo = 0; cut_hi = 1; empty_stream = true;
            HIP_TRY(query());
        }
    }
    n_members_all = h_sc->n_members;
    if (n_members_all == 0) return fail(err, errlen, RGX_ERR_OPEN, "%s", kMsgOpen);     // offset 0 is not a BGZF member
    total_all = h_sc->total_inflated;
    first_member = seek ? h_sc->q_index[0] : 0;                                    // == n_members_all when the seek target is no member
    stop = std::min(h_sc->stop, n_members_all);
    memcpy(q_upos, h_sc->q_upos, sizeof q_upos);
    mark("member discovery (2 syncs)");

    return kGoOn;
}

int EventsRun::stage_range_and_inflate() {
    // -- member range of this call ---------------------------------------------------------------------------------------------
    DevBuf &b_arena = c->buf(Buf::arena);
    member_range(cut_lo, cut_hi, h_sc->q_index, stop, n_members_all, chunked, path.to_file_end, m_lo, m_hi);
    // only a byte range of the file went up (a shard of a shared scan): it must hold every member of this call's range
    if (overlap && (up.lo || up.hi < bam_len) && m_hi > m_lo && !upload_covers_members(hm.data(), m_lo, m_hi, up.lo, up.hi)) {
        mark("shard range does not cover its members: whole-file upload");
        return restart(Restart::shard_range_uncovered);
    }
    // arena offsets of the range ends
    uint64_t upos_hi = 0;
    HIP_TRY(upos_of(m_lo, upos_lo));
    HIP_TRY(upos_of(m_hi, upos_hi));
    total = upos_hi - upos_lo;
    n_range = m_hi - m_lo;
    HIP_TRY(b_arena.ensure(total + 256));
    HIP_TRY(hipEventRecord(c->ev[0], st));
    DevBuf &b_lens = c->buf(Buf::inflate_scratch);
    HIP_TRY(b_lens.ensure(inflate_scratch_bytes(std::max<uint32_t>(n_range, 64))));
    // with a seek, the members in front of its target are only inflated for the header's sake (same launch): their failures end nothing
    const uint32_t ignore_below = (seek && first_member < n_members_all && first_member > m_lo) ? first_member - m_lo : 0;
    d_bad = nullptr;                                 // region queries: which members of the range did not inflate (every chunk has its own end of stream)
    if (chunked && !chunks.empty() && n_range) {
        DevBuf &b_bad = c->buf(Buf::bad_members);
        HIP_TRY(b_bad.ensure((size_t)n_range + 64));
        d_bad = b_bad.as<uint8_t>();
        HIP_TRY(hipMemsetAsync(d_bad, 0, n_range, st));
    }
    const int pairs = inflate_plan_for(bam_len, total_all);      // (the whole file's ratio: a range of it is the same kind of payload)
    // (early tail: the second of two gated launches is still running on a side stream; whoever reads its part of the arena, or the launch's
    //  verdict, first makes the pipeline's stream wait for it)
    c->launch_timed = false;
    auto timed_launch = [&](hipStream_t q, bool piece, InflateGate gate) {      // the call's whole-range launch, with its own pair of events on its own stream
        if (c->link) { c->chip_hold.take(&c->link->chip); mark("the chip's DEFLATE turn is ours"); }
        (void)hipEventRecord(c->ev_launch[0], q);
        launch_inflate(d_bam, d_members + m_lo, n_range, b_arena.as<uint8_t>(), upos_lo, b_lens.as<uint32_t>(), &d_sc->inflate.first_bad, q,
            ignore_below, 0, piece, 0, d_bad, pairs, false, gate);
        (void)hipEventRecord(c->ev_launch[1], q);
        if (c->link && hipLaunchHostFunc(q, [](void *h) { ((TurnHold *)h)->give(); }, &c->chip_hold) != hipSuccess) { (void)hipGetLastError();
            c->chip_hold.give(); }
        c->launch_timed = true;
    };
    if (!overlap) timed_launch(st, false, InflateGate());
    else {
        // one launch per upload chunk, on the side streams: the members whose bytes (plus the decoder's 16-byte look-ahead) have arrived with
        // chunk j start as soon as its event fires, next to the launches of the chunks before it
        HIP_TRY(b_lens.ensure(inflate_scratch_bytes(std::max<uint32_t>(n_range, 64)) + up.end.size() * inflate_scratch_bytes(64)));
        HIP_TRY(hipEventRecord(c->ev_ready, st));
        for (auto &q : c->side) if (q) HIP_TRY(hipStreamWaitEvent(q, c->ev_ready, 0));
        unsigned used_side = 0;
        Carve w_lens(b_lens);                                   // (every per-chunk launch below takes its own scratch)
        if (gated) {
            // one launch on the pipeline's stream, now: its waves wait for their chunk's flag themselves (k_inflate_coop; a range the wave form
            // takes -- a few thousand members -- is one launch behind the last chunk)
            if (inflate_takes_coop(n_range)) {
                InflateGate gate;
                gate.flags = c->buf(Buf::gate_flags).as<uint32_t>(); gate.epoch = c->gate_epoch; gate.n_chunks = (uint32_t)up.end.size(); gate.lo = up.lo;
                    gate.chunk_bytes = gate_chunk;
                // Round 4, second half ("early tail"): the launch goes to a side stream and counts its finished waves per PART of the member list
                // (parts cut where upload chunks end, at multiples of the lane-sorting group); the pipeline's stream waits for part after part
                // (launch_wait_done) and frames, verifies and decodes the part of the arena behind it while the waves of the later parts still
                // run -- what is left behind the launch's end is the last part's framing and decode, not the whole file's.  (A member's own
                // chain puts the end of the launch 6-9 ms behind the last chunk's arrival, whatever the chip does meanwhile.)
                if (!early_cuts().empty() && !c->early_distrust && c->side[1] && up.end.size() >= 8 && !d_bad && !d_true_sizes)
                    early_parts = plan_early_parts(hm.data(), m_lo, m_hi, upos_lo, up.end.data(), up.end.size(), early_cuts(), overlap_knobs().early_min,
                        kInflateSortGroup);
                if (!early_parts.empty()) {
                    DevBuf &bd = c->buf(Buf::gate_done);
                    HIP_TRY(bd.ensure(64));
                    uint32_t *d_done = bd.as<uint32_t>();
                    hipStream_t q = c->side[1];
                    HIP_TRY(hipMemsetAsync(d_done, 0, 32, q));
                    gate.done = d_done;
                    for (size_t j = 0; j < early_parts.size(); ++j) gate.part_start[j] = early_parts[j].waves;
                    timed_launch(q, /*piece=*/true, gate);
                    HIP_TRY(hipEventRecord(c->ev_side[1], q));
                    split_ev = c->ev_side[1];
                    split_B = true;
                } else timed_launch(st, /*piece=*/true, gate);
            } else {
                while (up.recorded.load(std::memory_order_acquire) < up.end.size()) std::this_thread::yield();
                HIP_TRY(hipStreamWaitEvent(st, c->chunk_ev[up.end.size() - 1], 0));
                timed_launch(st, false, InflateGate());
            }
        }
        // (the gated launch took the whole range: no pieces)
        for (const Piece &pc : gated ? std::vector<Piece>() : plan_pieces(hm.data(), m_lo, m_hi, up.end.data(), up.end.size())) {
            const size_t j = pc.chunk;
            const uint32_t g_lo = pc.g_lo, g_hi = pc.g_hi;
            // (an event must have been recorded before a stream can wait on it)
            while (up.recorded.load(std::memory_order_acquire) <= j) std::this_thread::yield();
            if (up.err) return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: upload failed\n");
            // the pipeline's own stream is idle until the inflate is done: it takes every third piece (the runtime maps streams onto four
            // hardware queues round-robin; a third side stream would share its queue with the second: profiles/r02_overlap_timeline.txt)
            const bool own = j + 1 == up.end.size() || j >= (size_t)kSideStreams || !c->side[j];
            hipStream_t q = own ? st : c->side[j];
            if (!own) used_side |= 1u << j;
            uint32_t *lens = (uint32_t *)w_lens.u8(inflate_scratch_bytes(g_hi - g_lo)); CARVE_TRY(w_lens, "inflate_scratch");
            HIP_TRY(hipStreamWaitEvent(q, c->chunk_ev[j], 0));
            launch_inflate(d_bam, d_members + g_lo, g_hi - g_lo, b_arena.as<uint8_t>(), upos_lo, lens,
                &d_sc->inflate.first_bad, q, ignore_below, g_lo - m_lo, /*piece=*/true, 0, d_bad, pairs);
        }
        up.th.join();
        // (gated waves give up after ~2 s)
        if (up.err) { (void)hipStreamSynchronize(st); return fail(err, errlen, RGX_ERR_DEVICE, "regtools_amd: upload failed\n"); }
        for (unsigned k = 0; k < (unsigned)kSideStreams; ++k) if (used_side >> k & 1) { HIP_TRY(hipEventRecord(c->ev_side[k], c->side[k]));
            HIP_TRY(hipStreamWaitEvent(st, c->ev_side[k], 0)); }
        HIP_TRY(hipStreamWaitEvent(st, c->chunk_ev[up.end.size() - 1], 0));      // (later stages read the file too: barcodes, header)
    }
    HIP_TRY(hipEventRecord(c->ev[1], st));
    mark(gated && overlap && inflate_takes_coop(n_range) ? "launch inflate (gated)" : "launch inflate");

    return kGoOn;
}

