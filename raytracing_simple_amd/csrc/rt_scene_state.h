// rt_scene_state.h -- what a context currently holds of its scene, on the host: whether there are records and a camera, whether the tables
// and the hierarchy still describe the records, whether the duplicate flags on the device do, whether the feature plane is current.  One
// member function per thing that happens to a scene; rt_api / rt_scene / rt_bvh / rt_features report the event and everybody READS the
// fields, nothing else writes them (DESIGN.md section 5.13 has the rules as one table).  The blocks the fields speak of are rt::Scene's
// (rt_internal.h).  No HIP in here -- tests/test_scene_state_cpu.py drives the record through the API's sequences with the host compiler alone.
#pragma once

#include <cstdint>

namespace rt {

struct SceneState {
    bool have_scene = false;            // records are on the device (or on their way) and the tables were built from them at least once
    bool have_cam = false;
    bool tables_stale = false;          // rt_update_spheres_async has changed records since the tables and the hierarchy were built: refresh_tables() builds them
                                        // ONCE, on the stream of whatever reads them next, however many updates went by (200 moved spheres by 200 calls cost 200
                                        // rebuilds before: 353 ms a frame at 8192 spheres against 4.9 in one call -- profiles/r06_update_calls.jsonl).  Implies have_scene
    bool bvh_ok = false;                // the blob describes the records as last built
    bool have_dups = false;             // both flag arrays (device, staging) describe the current records, and some record is flagged
    bool features_current = false;      // formed by rt_features_async since the last rt_set_scene / rt_update_spheres_async / rt_set_camera
    uint32_t n_tree = 0;                // spheres inside the tree (the slots are padded to whole leaves); 0 without a hierarchy
    uint32_t n_dups = 0;                // flagged records; 0 unless have_dups

    bool renderable() const { return have_scene && have_cam; }
    bool needs_refresh() const { return tables_stale && have_scene; }
    bool has_hierarchy() const { return bvh_ok; }
    bool flags_on_device() const { return have_dups; }     // the device holds flags that say something: the next marking has to overwrite them, even with none

    // ---- rt_set_scene ----
    void same_records_set() { features_current = false; }  // the very records the context holds: whatever is set, the feature plane is current UNTIL the call
    void records_replaced() { features_current = false; }  // ... other records: before capacity and upload, so a call that fails there has ended the plane too
    void upload_failed() { have_scene = false; }            // the tables are in an unknown state: no scene until the next rt_set_scene
    void uploaded() { have_scene = true; }
    // ---- rt_update_spheres_async: the records go now, tables and hierarchy follow when something reads them ----
    void records_updated() { tables_stale = true; features_current = false; }
    void camera_set() { have_cam = true; features_current = false; }        // rt_set_camera
    void tables_built() { tables_stale = false; }           // tables AND hierarchy queued (a build that failed half-way stays stale: the next reader tries again)
    // ---- the hierarchy (rt_bvh.hip) ----
    void hierarchy_voided() { bvh_ok = false; n_tree = 0; }                 // a build begins, or the blob is gone
    void hierarchy_adopted(uint32_t tree_spheres) { bvh_ok = true; n_tree = tree_spheres; }     // a builder's blob is queued behind the records
    void duplicates_marked(uint32_t found) { have_dups = found != 0; n_dups = found; }         // (0: none, or the marking has only begun)
    void capacity_replaced() { hierarchy_voided(); have_dups = false; }     // the blocks sized by the capacity are new: neither blob nor flags; the records follow (rt_set_scene)
    void features_formed() { features_current = true; }     // rt_features_async
};

}  // namespace rt
