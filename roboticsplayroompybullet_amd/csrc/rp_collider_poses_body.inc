/* rp_collider_poses_body.inc - the body of k_collider_poses behind the block's early exits, shared TEXTUALLY with k_collider_poses_rows (rp_render_states): rp_render.cuh
 * includes it once into each kernel.  As an inlined function the same statements compiled to another k_collider_poses (other registers, other spills); included, the
 * kernel is instruction for instruction the one it was.  In scope where it is included: the kernel's m, tab, cnt, sub_goal, ee_pose, ghost_arm, vis, num; L (the
 * block's EnvLds), slot, lane; state and srow - the state record is row srow of state -; venv, the row of vis the colours come from (vis null: the baked ones); and
 * the constant SOLID.  SOLID = false: the sub-goal's words are overwritten for a SECOND pass whose records carry RC_GHOST.  SOLID = true (rp_render_states'
 * RP_GOAL_SOLID): the same words are overwritten before the ONE and only pass - the records are those of the row with these words replaced, opaque, without the ghost
 * flag, the toggles coloured by the goal's joint values - and ghost_arm is not looked at. */
  load_state(L, state, srow, lane);
  float* out = tab + (size_t)slot * RC_MAX * RC_STRIDE;
  const bool obj_ghosts = sub_goal && m->num_objects > 0;
  const int passes = SOLID ? 1 : ((obj_ghosts || ghost_arm) ? 2 : 1);
  int nrec = 0;
  for (int pass = 0; pass < passes; pass++) {
    if (!SOLID && pass == 1 && ghost_arm) {      /* the ghost arm's joints: rest pose, one IK call, the first six joints (environments.py:575-590 with from_init's pose) */
      const float* ga = ghost_arm + 8 * (size_t)slot;
      __syncthreads();
      if (lane == 0) {
        const int nrest = m->arm_type == RP_ARM_PANDA ? 8 : 6;
        for (int i = 0; i < nrest; i++) L.st[ST_Q + i] = m->rest[i];
      }
      __syncthreads();
      ChainQ cur;
#pragma unroll
      for (int j = 0; j < 7; j++) cur.q[j] = j < m->ee_chain ? L.st[ST_Q + j] : 0.f;
      Q4 gq; gq.x = ga[3]; gq.y = ga[4]; gq.z = ga[5]; gq.w = ga[6];
      const ChainQ sol = ik_solve(m, mk3(ga[0], ga[1], ga[2]), gq, cur, 20, lane & 15);
      __syncthreads();
      if (lane == 0) for (int i = 0; i < 6; i++) L.st[ST_Q + i] = sol.q[i];
      __syncthreads();
      if (ee_pose && lane < 8) ee_pose[12 * (size_t)num + 8 * (size_t)slot + lane] = L.st[ST_Q + lane];      /* (test hook rp_debug_ghost_joints: the ghost's joints behind the EE poses) */
    }
    if (pass == (SOLID ? 0 : 1) && obj_ghosts) {           /* the sub-goal's poses: objects [pos3 (quat4)] ..., then drawer y, door, button, dial (play ids) */
      __syncthreads();
      if (lane == 0) {
        const float* g = sub_goal + (size_t)slot * m->n_ag;
        int idx = 0;
        for (int b = 0; b < m->num_objects; b++) {
          float* f = &L.st[ST_FREE + 13 * b];
          for (int k = 0; k < 3; k++) f[k] = g[idx + k];
          idx += 3;
          if (m->use_orientation) { for (int k = 0; k < 4; k++) f[3 + k] = g[idx + k]; idx += 4; }
        }
        if (m->play) {
          L.st[ST_FREE + 13 * m->drawer_free + 1] = g[idx];
          for (int k = 0; k < m->n_j1; k++) L.st[ST_JQ + k] = g[idx + 1 + k];
        }
      }
      __syncthreads();
    }
    fk_bodies(m, L, lane);
    __syncthreads();
    if (pass == 0 && ee_pose && lane == 0) {        /* EE link pose for the gripper camera */
      const int eb = m->site_body[RP_SITE_EE];
      const M3 Rb = ldm3(&L.xR[9 * eb]);
      const V3 pos = ld3(&L.xp[3 * eb]) + mulv(Rb, ld3(m->site_pos[RP_SITE_EE]));
      const M3 Rs = mul(Rb, ldm3(m->site_rot[RP_SITE_EE]));
      float* e = ee_pose + 12 * slot;
      st3(e, pos);
      for (int k = 0; k < 9; k++) e[3 + k] = Rs.m[k];
    }
    const int cbody = lane < m->n_col ? m->col_body[lane] : 0;
    const bool mine = lane < m->n_col && (pass == 0 || (obj_ghosts && cbody > m->n_arm) || (ghost_arm && cbody >= 1 && cbody <= m->n_arm));    /* ghosts: free bodies and scene joints of a sub-goal, the arm's links of a ghost arm */
    const unsigned long long bal = __ballot(mine);
    if (mine) {
      const int r = nrec + __popcll(bal & ((1ull << lane) - 1ull));
      const Xf x = collider_xf(m, L, lane);
      float* o = out + r * RC_STRIDE;
      for (int k = 0; k < 9; k++) o[k] = x.R.m[k];
      st3(o + 9, x.p);
      st3(o + 12, ld3(m->col_he[lane]));
      const float* rgb = vis ? vis + (size_t)venv * (3 * m->n_col + VIS_TAIL) + 3 * lane : m->col_rgb[lane];
      float cr = rgb[0], cg = rgb[1], cb = rgb[2];
      const int tog = m->col_toggle[lane];
      if (tog == 1 && m->n_j1 > 1) { const bool on = L.st[ST_JQ + 1] < 0.025f; cr = 1.f; cg = on ? 0.f : 1.f; cb = on ? 0.f : 1.f; }
      if (tog == 2 && m->n_j1 > 2) { const bool on = dial01(L.st[ST_JQ + 2]) < 0.5f; cr = 1.f; cg = on ? 0.f : 1.f; cb = on ? 0.f : 1.f; }
      o[15] = cr; o[16] = cg; o[17] = cb;
      o[18] = __int_as_float(m->col_type[lane] | (pass == 1 ? RC_GHOST : 0) | ((m->hpl && m->hpl_cnt[lane] > 0) ? RC_HULL : 0));
      o[19] = __int_as_float((m->col_link[lane] << 8) | lane);
    }
    nrec += __popcll(bal);
  }
  if (lane == 0) cnt[slot] = nrec;
