! Driver of tools/make_golden_gribin.py.  Unlike tools/gribout_driver.F90 it calls NO routine of the reference: the statements of the GRIB read
! (grib2wgrid.F90:771-775 the un-scaling, 793-802 the full copy into FIELD; getspec.F90:458-462 the gather, 548-552 the store with
! ZMISS -> EPSMIN) sit inside GRIB2WGRID and GETSPEC, which are bound to eccodes and MPL and do not compile alone.  This program is the project's
! own few lines around Fortran's own `**`: what it pins is the compiler's evaluation of 10**(V - |PPREC|) - PPEPS in the working precision
! (both are built, by oracle/ref_build.py::build_driver as every driver is), through a two-dimensional FIELD as the reference goes, not a compiled reference routine.
! Input  (stream, little endian): NGX, NGY, NPTS, NVAL, NFLD, IUNSCALE (int32); PPEPS, PPREC, ZMISS, EPSMIN (real64); NLONRGG(NGY), IXLG(NPTS),
!        KXLT(NPTS) (int32); V8(NVAL,NFLD) (real64), the decoded vectors.  Every real is representable in the working precision.
! Output (stream): FL(NPTS) per field (real64): the working-precision result, widened.
PROGRAM GRIBIN_DRIVER
  USE PARKIND1, ONLY : JWIM => JPIM, JWRB => JPRB      ! oracle/ref_stubs.F90: the kinds parkind_wave.F90 takes (-DREF_SINGLE: single)
  IMPLICIT NONE
  INTEGER(KIND=JWIM) :: H(6), NGX, NGY, NPTS, NVAL, NFLD, IUNSCALE, IFLD, IJ, J, I, L
  REAL(KIND=8) :: R(4)
  REAL(KIND=JWRB) :: PPEPS, PPREC, ZMISS, EPSMIN
  INTEGER(KIND=JWIM), ALLOCATABLE :: NLONRGG(:), IXLG(:), KXLT(:)
  REAL(KIND=8), ALLOCATABLE :: V8(:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: V(:), FIELD(:,:), WORK(:), FL(:)
  CHARACTER(LEN=512) :: FIN, FOUT

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) H, R
  NGX = H(1); NGY = H(2); NPTS = H(3); NVAL = H(4); NFLD = H(5); IUNSCALE = H(6)
  PPEPS = REAL(R(1), JWRB); PPREC = REAL(R(2), JWRB); ZMISS = REAL(R(3), JWRB); EPSMIN = REAL(R(4), JWRB)
  ALLOCATE(NLONRGG(NGY), IXLG(NPTS), KXLT(NPTS), V8(NVAL,NFLD), V(NVAL), FIELD(NGX,NGY), WORK(NPTS), FL(NPTS))
  READ(11) NLONRGG, IXLG, KXLT, V8

  DO IFLD = 1, NFLD
    V(:) = REAL(V8(:,IFLD), JWRB)
    ! the decoded values back on their scale; a missing value stays missing
    IF (IUNSCALE /= 0) THEN
      DO L = 1, NVAL
        IF (V(L) /= ZMISS) V(L) = 10.0_JWRB**(V(L) - ABS(PPREC)) - PPEPS
      ENDDO
    ENDIF
    ! the vector into the grid, north to south, every row from the first value on; what no value reaches is marked
    FIELD(:,:) = -HUGE(ZMISS)
    L = 0
    DO J = 1, NGY
      DO I = 1, NLONRGG(NGY-J+1)
        L = L + 1
        FIELD(I,J) = V(L)
      ENDDO
    ENDDO
    ! the grid into the block, then into the spectrum's slot for this field
    DO IJ = 1, NPTS
      WORK(IJ) = FIELD(IXLG(IJ), NGY-KXLT(IJ)+1)
    ENDDO
    FL(:) = WORK(:)
    DO IJ = 1, NPTS
      IF (FL(IJ) == ZMISS) FL(IJ) = EPSMIN
    ENDDO
    WRITE(12) REAL(FL, 8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM GRIBIN_DRIVER
