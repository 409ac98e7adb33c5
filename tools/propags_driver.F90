! Driver of tools/make_golden_propags.py: calls the reference's PROPDOT (with GRADI) and PROPAGS on the cases of a stream file and writes what they return.
! It is built by oracle/ref_build.py::build_driver: the routines and the modules they use are the reference's own files, compiled unmodified in both
! precisions, behind the stand-ins of oracle/ref_stubs.F90; the driver holds no module of its own.  The program fills the module variables the routines
! read (the USE lines of propags.F90:80-96, propdot.F90:67-73 and gradi.F90:65-70) from the file.
! The one routine the driver supplies in place of the reference's is the external CHECKCFL below: the reference's aborts where a number exceeds 1; this one
! records its eleven arguments per (K, M = 1) -- PROPAGS calls it once per direction, in the order of the directions -- so that the CFL numbers of the
! unmodified PROPAGS are had, those above 1 included.  build_driver cuts checkcfl.intfb.h from it.
! Input  (stream, little endian): N, NANG, NFRE_RED, NGY (int32); FR(NFRE_RED), SINTH(NANG), COSTH(NANG), then DELTH, R, ZPI, PI (real64); KXLT(N), KLON(N,2),
!        KLAT(N,2,2) (int32, 1-based, the land row is N+1); then cases, each led by an int32 1 (0 ends the file):
!          ICASE, IRGG, IREFRA, IDELPRO, LOBS (int32); DELPHI (real64); DELLAM(NGY), SINPH(NGY), COSPH(NGY), WLAT(N,2); DELLAM1, COSPHM1, DEPTH, U, V (N+1 each);
!          CGROUP, OMOSNH2KD, WAVNUM (N+1,NFRE_RED each); with LOBS /= 0 OBSLAT(N,NFRE_RED,2), OBSLON(N,NFRE_RED,2); F1(N+1,NANG,NFRE_RED)
!        Every real is representable in the working precision.
! Output (stream, real64: the working-precision results, widened), per case: F3(N,NANG,NFRE_RED), THDD(N,NANG), THDC(N,NANG), SDOT(N,NANG,NFRE_RED),
!        CFL(N,NANG,11), the number of CHECKCFL calls.
PROGRAM PROPAGS_DRIVER
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  USE YOWDRVTYPE, ONLY : WVGRIDGLO
  USE YOWCURR, ONLY : LLCHKCFL
  USE YOWFRED, ONLY : FR, DELTH, COSTH, SINTH
  USE YOWGRID, ONLY : DELPHI, DELLAM, SINPH, COSPH
  USE YOWMAP, ONLY : IRGG, NIBLO
  USE YOWPARAM, ONLY : NANG, NFRE, NFRE_RED
  USE YOWPCONS, ONLY : PI, ZPI, R
  USE YOWREFD, ONLY : THDD, THDC, SDOT
  USE YOWSTAT, ONLY : IDELPRO, ICASE, IREFRA
  USE YOWUBUF, ONLY : KLAT, KLON, WLAT, OBSLAT, OBSLON
  IMPLICIT NONE
#include "propdot.intfb.h"
#include "propags.intfb.h"
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER, PARAMETER :: MAXP = 256, MAXK = 64
  REAL(KIND=R8) :: CFLREC(MAXP, MAXK, 11)
  INTEGER :: NCALL
  COMMON /PGREC/ CFLREC, NCALL
  INTEGER(KIND=JWIM) :: N, NGY, OP, LOBS
  TYPE(WVGRIDGLO) :: BLK2GLO
  INTEGER(KIND=JWIM), ALLOCATABLE, TARGET :: KXLT(:)
  REAL(KIND=R8) :: S(4), D8
  REAL(KIND=R8), ALLOCATABLE :: A8(:), G8(:), W8(:,:), P8(:,:), E8(:,:,:), O8(:,:,:,:), F8(:,:,:)
  REAL(KIND=JWRB), ALLOCATABLE :: F1(:,:,:), F3(:,:,:), P(:,:), E(:,:,:)
  CHARACTER(LEN=512) :: FIN, FOUT

  CALL GET_COMMAND_ARGUMENT(1, FIN)
  CALL GET_COMMAND_ARGUMENT(2, FOUT)
  OPEN(11, FILE=TRIM(FIN), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='OLD')
  OPEN(12, FILE=TRIM(FOUT), ACCESS='STREAM', FORM='UNFORMATTED', STATUS='REPLACE')
  READ(11) N, NANG, NFRE_RED, NGY
  IF (N > MAXP .OR. NANG > MAXK) ERROR STOP 'SIZE'
  NFRE = NFRE_RED
  NIBLO = N
  ALLOCATE(FR(NFRE_RED), SINTH(NANG), COSTH(NANG), A8(NFRE_RED))
  READ(11) A8
  FR = REAL(A8, JWRB)
  DEALLOCATE(A8)
  ALLOCATE(A8(NANG))
  READ(11) A8
  SINTH = REAL(A8, JWRB)
  READ(11) A8
  COSTH = REAL(A8, JWRB)
  READ(11) S
  DELTH = REAL(S(1), JWRB)
  R = REAL(S(2), JWRB)
  ZPI = REAL(S(3), JWRB)
  PI = REAL(S(4), JWRB)
  ALLOCATE(KXLT(N), KLON(N,2), KLAT(N,2,2), WLAT(N,2), OBSLAT(N,NFRE_RED,2), OBSLON(N,NFRE_RED,2))
  READ(11) KXLT, KLON, KLAT
  BLK2GLO%KXLT => KXLT
  ALLOCATE(DELLAM(NGY), SINPH(NGY), COSPH(NGY), G8(NGY), W8(N,2), P8(N+1,5), P(N+1,5), E8(N+1,NFRE_RED,3), E(N+1,NFRE_RED,3), O8(N,NFRE_RED,2,2))
  ALLOCATE(F8(N+1,NANG,NFRE_RED), F1(N+1,NANG,NFRE_RED), F3(N+1,NANG,NFRE_RED))
  ALLOCATE(THDD(N,NANG), THDC(N,NANG), SDOT(N,NANG,NFRE_RED))
  LLCHKCFL = .TRUE.
  DO
    READ(11) OP
    IF (OP == 0) EXIT
    READ(11) ICASE, IRGG, IREFRA, IDELPRO, LOBS, D8
    DELPHI = REAL(D8, JWRB)
    READ(11) G8
    DELLAM = REAL(G8, JWRB)
    READ(11) G8
    SINPH = REAL(G8, JWRB)
    READ(11) G8
    COSPH = REAL(G8, JWRB)
    READ(11) W8, P8, E8
    WLAT = REAL(W8, JWRB)
    P = REAL(P8, JWRB)
    E = REAL(E8, JWRB)
    OBSLAT = 1.0_JWRB
    OBSLON = 1.0_JWRB
    IF (LOBS /= 0) THEN
      READ(11) O8
      OBSLAT = REAL(O8(:,:,:,1), JWRB)
      OBSLON = REAL(O8(:,:,:,2), JWRB)
    ENDIF
    READ(11) F8
    F1 = REAL(F8, JWRB)
    F3 = 0.0_JWRB
    THDD = 0.0_JWRB
    THDC = 0.0_JWRB
    SDOT = 0.0_JWRB
    CFLREC = 0.0_R8
    NCALL = 0
    ! propag_wam.F90:341-362: the dot terms with refraction, then the scheme
    IF (IREFRA /= 0) THEN
      CALL PROPDOT(1_JWIM, N, 1_JWIM, N, BLK2GLO, E(:,:,3), E(:,:,1), E(:,:,2), P(:,2), P(:,3), P(:,4), P(:,5), THDC, THDD, SDOT)
    ENDIF
    CALL PROPAGS(F1, F3, 1_JWIM, N, 1_JWIM, N, BLK2GLO, P(:,3), E(:,:,1), E(:,:,2), P(:,1), P(:,2), P(:,4), P(:,5), .TRUE.)
    WRITE(12) REAL(F3(1:N,:,:), R8), REAL(THDD, R8), REAL(THDC, R8), REAL(SDOT, R8), CFLREC(1:N,1:NANG,:), REAL(NCALL, R8)
  ENDDO
  CLOSE(11)
  CLOSE(12)
END PROGRAM PROPAGS_DRIVER

SUBROUTINE CHECKCFL (KIJS, KIJL, DEPTH, DTC, CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2, CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM)
  USE PARKIND_WAVE, ONLY : JWIM, JWRB
  IMPLICIT NONE
  INTEGER(KIND=JWIM), INTENT(IN) :: KIJS, KIJL
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: DEPTH
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: DTC
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: CFLEA, CFLWE, CFLNO, CFLSO, CFLNO2
  REAL(KIND=JWRB), DIMENSION(KIJS:KIJL), INTENT(IN) :: CFLSO2, CFLTP, CFLTM, CFLOP, CFLOM
  INTEGER, PARAMETER :: R8 = SELECTED_REAL_KIND(13, 300)
  INTEGER, PARAMETER :: MAXP = 256, MAXK = 64
  REAL(KIND=R8) :: CFLREC(MAXP, MAXK, 11)
  INTEGER :: NCALL
  COMMON /PGREC/ CFLREC, NCALL
  INTEGER(KIND=JWIM) :: IJ, K
  NCALL = NCALL + 1
  K = NCALL
  IF (K > MAXK) ERROR STOP 'CHECKCFL CALLS'
  DO IJ = KIJS, KIJL
    CFLREC(IJ,K,1) = REAL(DTC(IJ), R8)
    CFLREC(IJ,K,2) = REAL(CFLEA(IJ), R8)
    CFLREC(IJ,K,3) = REAL(CFLWE(IJ), R8)
    CFLREC(IJ,K,4) = REAL(CFLNO(IJ), R8)
    CFLREC(IJ,K,5) = REAL(CFLSO(IJ), R8)
    CFLREC(IJ,K,6) = REAL(CFLNO2(IJ), R8)
    CFLREC(IJ,K,7) = REAL(CFLSO2(IJ), R8)
    CFLREC(IJ,K,8) = REAL(CFLTP(IJ), R8)
    CFLREC(IJ,K,9) = REAL(CFLTM(IJ), R8)
    CFLREC(IJ,K,10) = REAL(CFLOP(IJ), R8)
    CFLREC(IJ,K,11) = REAL(CFLOM(IJ), R8)
  ENDDO
END SUBROUTINE CHECKCFL
