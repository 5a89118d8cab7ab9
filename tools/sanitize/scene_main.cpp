// What a context holds of its scene (csrc/rt_scene_state.h) alone, under AddressSanitizer + UndefinedBehaviorSanitizer: the record has no HIP, so the
// program drives it through the transitions in the order the API's calls report them (rt_api.hip, rt_scene.hip, rt_bvh.hip, rt_features.hip).
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -I raytracing_simple_amd/csrc tools/sanitize/scene_main.cpp -o scene_san && ./scene_san
// One line per case ("ok <case>" / "FAILED <case>: ..."), then "scene: clean"; the exit status is the number of failed cases.
#include <cstdio>

#include "rt_scene_state.h"

using rt::SceneState;

namespace {
int g_failed = 0;
void check(const char *name, bool ok, const char *what) {
    if (ok) printf("ok %s\n", name);
    else { printf("FAILED %s: %s\n", name, what); g_failed += 1; }
}

// ---- the calls, as the library makes them (what the device does in between is left out) ----
// rt_bvh.hip mark_duplicates: *uploaded = the flags went to the device
void mark_duplicates(SceneState &s, uint32_t found, bool *uploaded) {
    const bool had = s.flags_on_device();
    s.duplicates_marked(0);
    *uploaded = !(found == 0 && !had);
    if (*uploaded) s.duplicates_marked(found);
}
// rt_scene.hip build_tables -> rt_bvh.hip build_bvh_tables: a scene of which `n_tree` records go into a tree (0: no hierarchy); ok = false: a HIP call failed half-way
bool build_tables(SceneState &s, uint32_t n_tree, uint32_t dups, bool ok = true, bool *dup_upload = nullptr) {
    s.hierarchy_voided();
    if (n_tree) {
        bool up = false;
        mark_duplicates(s, dups, &up);
        if (dup_upload) *dup_upload = up;
        if (!ok) return false;
        s.hierarchy_adopted(n_tree);
    }
    if (ok) s.tables_built();
    return ok;
}
// rt_set_scene with other records: `grows` = ensure_scene_capacity replaced the blocks
bool set_scene(SceneState &s, uint32_t n_tree, uint32_t dups, bool grows = false, bool upload_ok = true, bool *dup_upload = nullptr) {
    s.records_replaced();
    if (grows) s.capacity_replaced();
    const bool ok = build_tables(s, n_tree, dups, upload_ok, dup_upload);
    if (ok) s.uploaded();
    else s.upload_failed();
    return ok;
}
// rt_update_spheres_async: false = refused (RT_ERR_STATE)
bool update(SceneState &s) {
    if (!s.have_scene) return false;
    s.records_updated();                // the call, then upload_spheres' device-resident branch
    s.records_updated();
    return true;
}
// refresh_tables: true = it built
bool refresh(SceneState &s, uint32_t n_tree, uint32_t dups, bool ok = true) {
    if (!s.needs_refresh()) return false;
    build_tables(s, n_tree, dups, ok);
    return true;
}
}  // namespace

int main() {
    {
        SceneState s;
        bool ok = !s.renderable() && !s.needs_refresh() && !s.has_hierarchy() && !s.flags_on_device();
        s.camera_set();
        ok = ok && !s.renderable() && s.have_cam;
        SceneState t;
        set_scene(t, 0, 0);
        ok = ok && !t.renderable() && t.have_scene;
        set_scene(s, 0, 0);
        t.camera_set();
        check("renderable_needs_scene_and_camera", ok && s.renderable() && t.renderable(), "renderable before both were set, or not after");
    }
    {
        SceneState s;
        set_scene(s, 200, 1);
        s.camera_set();
        s.features_formed();
        const SceneState before = s;
        s.same_records_set();
        const bool ok = !s.features_current && before.features_current && s.have_scene == before.have_scene && s.have_cam == before.have_cam &&
                        s.tables_stale == before.tables_stale && s.bvh_ok == before.bvh_ok && s.have_dups == before.have_dups && s.n_tree == before.n_tree &&
                        s.n_dups == before.n_dups && s.n_tree == 200 && s.n_dups == 1;
        check("identical_set_scene_ends_the_features_only", ok, "another field moved, or the plane stayed current");
    }
    {
        SceneState s;
        set_scene(s, 0, 0);
        bool ok = update(s);
        ok = ok && !set_scene(s, 0, 0, false, false) && !s.have_scene && !s.renderable();
        ok = ok && !update(s) && !s.needs_refresh();
        ok = ok && set_scene(s, 0, 0) && s.have_scene && update(s);
        check("failed_upload_leaves_no_scene_and_refuses_updates", ok, "a scene after a failed upload, or an update taken without one");
    }
    {
        SceneState s;
        set_scene(s, 0, 0);
        bool ok = !s.tables_stale && !s.needs_refresh();
        for (int k = 0; k < 3; ++k) ok = ok && update(s) && s.tables_stale && s.needs_refresh();
        ok = ok && refresh(s, 0, 0, false) && s.tables_stale && s.needs_refresh();      // failed half-way: the next reader tries again
        ok = ok && refresh(s, 0, 0) && !s.tables_stale && !s.needs_refresh();
        ok = ok && !refresh(s, 0, 0);                                                   // built once for all the updates
        check("updates_leave_tables_stale_until_a_rebuild_succeeds", ok, "stale cleared by a failed build, or kept by a good one");
    }
    {
        SceneState s;
        set_scene(s, 200, 2);
        s.camera_set();
        bool ok = s.has_hierarchy() && s.flags_on_device() && s.n_tree == 200 && s.n_dups == 2;
        s.capacity_replaced();
        ok = ok && !s.has_hierarchy() && !s.flags_on_device() && s.n_tree == 0 && s.have_scene && s.have_cam && s.renderable();
        check("replaced_capacity_voids_hierarchy_and_flags_not_the_scene", ok, "the blob or the flags survived their blocks, or the scene did not");
    }
    {
        SceneState s;
        bool up = false;
        set_scene(s, 200, 0, false, true, &up);
        bool ok = !up && !s.flags_on_device();                          // nothing to say, nothing on the device
        set_scene(s, 200, 3, false, true, &up);
        ok = ok && up && s.flags_on_device() && s.n_dups == 3;
        set_scene(s, 200, 0, false, true, &up);
        ok = ok && up && !s.flags_on_device() && s.n_dups == 0;         // the now-empty flags overwrite the old ones ...
        set_scene(s, 200, 0, false, true, &up);
        ok = ok && !up && !s.flags_on_device();                         // ... once
        set_scene(s, 200, 3, false, true, &up);
        set_scene(s, 300, 0, true, true, &up);                          // new blocks hold no flags: nothing to overwrite
        ok = ok && !up;
        check("empty_flags_are_uploaded_once_after_a_scene_with_duplicates", ok, "the found == 0 && !had rule");
    }
    {
        SceneState s;
        set_scene(s, 0, 0);
        s.camera_set();
        bool ok = !s.features_current;
        s.features_formed();
        ok = ok && s.features_current;
        s.same_records_set();
        ok = ok && !s.features_current;
        s.features_formed();
        set_scene(s, 0, 0);
        ok = ok && !s.features_current;
        s.features_formed();
        update(s);
        ok = ok && !s.features_current;
        s.features_formed();
        s.camera_set();
        ok = ok && !s.features_current;
        s.features_formed();
        // ... and with nothing else: a rebuild, a voided and an adopted hierarchy, a marking, new blocks
        refresh(s, 0, 0);
        s.tables_built();
        s.hierarchy_voided();
        s.hierarchy_adopted(100);
        s.duplicates_marked(1);
        s.capacity_replaced();
        s.uploaded();
        ok = ok && s.features_current;
        check("features_end_with_three_calls_and_nothing_else", ok, "the plane stayed current across a call that ends it, or ended without one");
    }
    {
        SceneState s;
        s.hierarchy_adopted(150);
        bool ok = s.has_hierarchy() && s.n_tree == 150;
        s.hierarchy_voided();
        ok = ok && !s.has_hierarchy() && s.n_tree == 0;
        s.hierarchy_adopted(777);
        ok = ok && s.has_hierarchy() && s.n_tree == 777;
        check("hierarchy_adopted_after_voided_reports_n_tree", ok, "n_tree");
    }
    if (g_failed == 0) printf("scene: clean\n");
    return g_failed;
}
