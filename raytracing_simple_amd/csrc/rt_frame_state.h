// rt_frame_state.h -- what the progressive frame of a context currently IS, on the host: its pass number, which seed stream the next launch
// reads, whether the packed pixels are up to date, the launch count, and the tile bookkeeping of adaptive sampling (rt_tiles.hip).  One member
// function per thing that happens to a frame; the calls of rt_api / rt_state / rt_tiles / rt_compare / rt_denoise / rt_launch / rt_debug / rt_multi
// report the event and READ the fields, nothing else writes them (DESIGN.md section 5.10 has the rules as one table).  No HIP in here --
// tests/test_frame_state_cpu.py drives the record through its sequences with the host compiler alone.
#pragma once

#include <cstdint>

namespace rt {

struct FrameState {
    int current_sample = 0;             // passes the running average holds (a ragged frame: at its front)
    bool seeds_default = false;         // the next launch reads the pristine default stream in place (d_seeds0), not d_seeds
    bool seeds_custom = false;          // d_seeds was last filled by rt_seed_stream_async / rt_write_state, not from the default stream
    bool pixels_current = true;         // the packed pixel buffer holds the frame of the running average
    uint64_t launches = 0;              // since the last reset
    double last_ms = 0.0;               // device time of the last blocking launch
    // Adaptive sampling.  A GROUP is the 8x8 tiles 4g .. 4g+3 of one tile row; it is rendered whole or not at all, so its tiles hold one pass count.
    bool ragged = false;                // some tile holds fewer passes than current_sample (only then does TileSubset::d_passes mean anything)
    bool have_selection = false;        // rt_select_tiles' flags and counts are in hand
    uint32_t counts[2] = { 0, 0 };      // selected groups, the 8x8 tiles they cover
    uint64_t selection_serial = 0;      // counts rt_select_tiles calls
    // what the subset launch's tile list was built from: it is rebuilt only when one of these changes (list_is_stale)
    bool list_valid = false, list_by_order = false;
    uint64_t list_serial = 0;
    uint32_t list_tiles = 0;            // launch tiles of the instance's shape
    uint32_t list_slots = 0;            // entries: the launch's grid.x * grid.y
    // The error of the filtered frame (rt_denoise.hip rt_denoise_pair_async): the call that made this context's cross-filtered plane, numbered per
    // process from 1 and shared by the two contexts of that call; 0 while the plane is stale -- never made, or the colour plane has moved since
    uint64_t filtered_pair = 0;
    // ... and, while the plane is stale for ONE reason only -- subset launches of the selection still in hand have moved the colour plane of the
    // selected groups -- the call it was current under: what rt_denoise_pair_tiles_async refreshes from.  0 otherwise
    uint64_t filtered_behind = 0;
    // the compacted list of selected groups that call's kernel walks (TileSubset::d_groups): the selection it was built from, 0 = none
    uint64_t group_list_serial = 0;
    // Temporal reprojection (rt_reproject.hip): the temporal plane beside the colour plane was formed by rt_reproject_async and nothing has moved the
    // colour plane since.  The plane is CURRENT while this holds and the scene's feature plane is current too (SceneState::features_current)
    bool temporal_current = false;
    // The edge-avoiding wavelet filter (rt_atrous.hip): the filtered plane was formed by rt_atrous_async from the temporal plane -- or, where none was
    // current, from the colour plane -- and neither has moved since.  CURRENT while this holds and the scene's feature plane is current too
    bool atrous_current = false;
    // Temporal luminance moments (rt_reproject.hip): the reprojection that formed the temporal plane formed the moments plane too.  CURRENT while both hold
    bool moments_formed = false;

    // at pass 0 the next launch would read the default stream (nothing but a custom stream or a written state puts another one there)
    bool on_default_stream() const { return seeds_default || !seeds_custom; }
    bool list_is_stale(bool by_order, uint32_t tiles) const { return !list_valid || list_serial != selection_serial || list_tiles != tiles || list_by_order != by_order; }
    // the cross-filtered planes of this context and of `other` are current and were made by one rt_denoise_pair_async call
    bool filtered_with(const FrameState &other) const { return filtered_pair != 0 && filtered_pair == other.filtered_pair; }
    // ... were so, and nothing but subset launches of the selections both still hold has moved either colour plane since
    bool filtered_behind_with(const FrameState &other) const {
        return filtered_behind != 0 && filtered_behind == other.filtered_behind && have_selection && other.have_selection;
    }
    bool group_list_is_stale() const { return group_list_serial == 0 || group_list_serial != selection_serial; }

    // ---- resets and written states: a whole frame at one pass number again ----
    // rt_reset: the restore kernel copies the default stream into d_seeds and clears the pixels
    void reset_blocking() { restart(0); seeds_default = seeds_custom = false; pixels_current = true; }
    void reset_in_place() { restart(0); seeds_default = true; }                     // rt_reset_async: nothing is copied, the next launch reads d_seeds0
    void custom_seeds_written() { seeds_default = false; seeds_custom = true; }     // rt_seed_stream_async, stream id != 0, after its reset
    // rt_write_state; without seeds the default stream is read in place, and the frame is packed from the written plane when somebody reads it --
    // beyond pass 0: refresh_pixels packs nothing while current_sample is 0 (the plane holds nothing), and the packed pixels are unspecified there
    void state_written(int pass, bool with_seeds) { restart(pass); seeds_default = !with_seeds; seeds_custom = with_seeds; pixels_current = false; }
    void debug_reset_by_copy() { current_sample = 0; seeds_default = seeds_custom = false; }    // the round-1 reset (rt_debug.hip): seeds and pass, nothing else

    // ---- launches ----
    void launched(int n_samples, bool pixel_store) { advance(n_samples); pixels_current = pixel_store; filtered_behind = 0; }    // a whole-frame launch
    void launched_subset(int n_samples, bool pixel_store, bool all_groups) {    // (the tiles left out keep the packed pixels they had)
        const uint64_t was = filtered_pair != 0 ? filtered_pair : filtered_behind;      // current, or behind by launches of this same selection already
        advance(n_samples);
        filtered_behind = was;          // the cross-filtered plane is one selection behind: the groups left out hold what it held
        pixels_current = pixel_store && (all_groups || pixels_current);
        ragged = !all_groups;           // every group selected means every group at the front: the frame stays (or is again) whole
    }
    void default_seeds_copied() { seeds_default = false; }      // a subset launch after an in-place reset: the tiles it leaves out hold the default stream too
    void timed(double ms) { last_ms = ms; }                     // a blocking launch's device time
    void front_follows(int pass) { current_sample = pass; }     // the front record of a multi-device context mirrors its shards' count (rt_multi.hip)

    // ---- selection and tile list ----
    void order_resorted() { list_valid = false; }               // a subset launch's list follows the heavy-first order
    // the flags are being rewritten: no selection until the counts are back, and a plane that was behind the old selection cannot be refreshed by the new one
    void selection_started() { have_selection = false; list_valid = false; filtered_behind = 0; }
    void selection_landed(uint32_t groups, uint32_t tiles) { counts[0] = groups; counts[1] = tiles; selection_serial += 1; have_selection = true; }
    void list_built(bool by_order, uint32_t tiles, uint32_t slots) {
        list_valid = true; list_by_order = by_order; list_serial = selection_serial; list_tiles = tiles; list_slots = slots;
    }
    void group_list_built() { group_list_serial = selection_serial; }          // rt_denoise_pair_tiles_async: once per selection

    // ---- the colour plane written by something else than a launch: rt_read_pixels packs it ----
    void merged(int total) { current_sample = total; have_selection = false; pixels_current = false; filtered_behind = 0; colour_plane_moved(); }     // (a selection was made at another pass number)
    void merged_by_tile(int total) { merged(total); ragged = true; list_valid = false; }                    // every tile by its own weights: dst's front has moved
    void colours_replaced() { pixels_current = false; filtered_behind = 0; colour_plane_moved(); }     // rt_denoise_async
    void pixels_packed() { pixels_current = true; }             // refresh_pixels
    // rt_denoise_pair_async: the cross-filtered plane beside the colour plane is current, until anything moves the colour plane (a launch, a reset,
    // a written state, a merge or a filter into it); nothing else of the frame changes
    void pair_filtered(uint64_t call) { filtered_pair = call; filtered_behind = 0; }
    // rt_denoise_pair_tiles_async: the selected groups' part of a plane that was one selection behind has been formed again -- current, under a new id
    void pair_tiles_refreshed(uint64_t call) { pair_filtered(call); }
    // rt_reproject_async into this context: its temporal plane is current, until anything moves the colour plane (the same events that end the
    // cross-filtered plane) or ends the feature plane (the scene's record); nothing else of the frame changes.  `with_moments`: the call formed the
    // moments plane beside it (rt_set_temporal_moments on for this context).  A plane filtered from the temporal plane that was is not a filter of this one
    void reprojected(bool with_moments = false) { temporal_current = true; moments_formed = with_moments; atrous_current = false; }
    // rt_features_async forms a feature plane where none was current: a temporal plane formed under the one that ended does not come back with it
    void features_reformed() { temporal_current = atrous_current = moments_formed = false; }
    // rt_atrous_async: the filtered plane is current, until any event that ends the temporal plane, a new reprojection into the context or a feature
    // plane formed again; nothing else of the frame changes -- the filter feeds nothing back
    void atrous_filtered() { atrous_current = true; }

private:
    // something has written the colour plane, or will before it is read again: every plane derived from it is stale.  (filtered_behind is each caller's own)
    void colour_plane_moved() { filtered_pair = 0; temporal_current = atrous_current = moments_formed = false; }
    // every tile holds `pass` passes; a selection does not outlive that, and the launch count starts again
    void restart(int pass) { current_sample = pass; launches = 0; last_ms = 0.0; ragged = have_selection = list_valid = false; filtered_behind = 0; colour_plane_moved(); }
    // a launch has written every seed pair it renders: the default stream is no longer read in place
    void advance(int n_samples) { current_sample += n_samples; launches += 1; seeds_default = false; colour_plane_moved(); }
};

}  // namespace rt
